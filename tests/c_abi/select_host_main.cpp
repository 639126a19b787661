// select_host_main.cpp -- the host half of the quantile selection (demc.jl_amd/csrc/demcz_select_host.h) as a stand-alone program,
// so that it can be built with -fsanitize=address,undefined and run on its own (tests/test_quantile_reference.py).
//
// Input file (native endianness): int64 S, d, nq; nq doubles (probabilities); d * S doubles (the draws of parameter p at
// [p S, (p + 1) S)).  The counting pass of the device is restated here on the host, per rank; demcz_quantile_plan,
// demcz_select_step and demcz_quantile_finish do the rest.  Output: one line per (parameter, probability), in that order, with
// the bit patterns of q, lower and upper in hexadecimal.  Exit code 3 + the status when a library function fails.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../demc.jl_amd/csrc/demcz_select_host.h"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int64_t hdr[3];
    if (std::fread(hdr, sizeof(int64_t), 3, f) != 3 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1 || hdr[2] > 64) { std::fclose(f); return 2; }
    const int64_t S = hdr[0];
    const int d = (int)hdr[1], nq = (int)hdr[2], nr = 2 * nq;
    std::vector<double> probs((size_t)nq), x((size_t)d * S);
    if (std::fread(probs.data(), sizeof(double), probs.size(), f) != probs.size() || std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) {
        std::fclose(f);
        return 2;
    }
    std::fclose(f);

    std::vector<int64_t> rlo((size_t)nq), rhi((size_t)nq), rank((size_t)d * nr), counts((size_t)256 * nr * d), nan((size_t)d, 0);
    std::vector<double> frac((size_t)nq);
    int32_t rc = demcz_quantile_plan(S, nq, probs.data(), rlo.data(), rhi.data(), frac.data());
    if (rc) { std::fprintf(stderr, "demcz_quantile_plan: %d\n", rc); return 3 + rc; }
    std::vector<uint64_t> key((size_t)d * S), prefix((size_t)d * nr, 0);
    for (int p = 0; p < d; ++p)
        for (int64_t i = 0; i < S; ++i) {
            const double v = x[(size_t)p * S + i];
            uint64_t b;
            std::memcpy(&b, &v, sizeof b);
            key[(size_t)p * S + i] = demcz::sel_key_of_bits(b);
            if (v != v) ++nan[p];
        }
    for (int p = 0; p < d; ++p)
        for (int j = 0; j < nq; ++j) { rank[p + (size_t)d * (2 * j)] = rlo[j]; rank[p + (size_t)d * (2 * j + 1)] = rhi[j]; }
    for (int shift = 56; shift >= 0; shift -= 8) {
        std::fill(counts.begin(), counts.end(), 0);
        for (int p = 0; p < d; ++p)
            for (int r = 0; r < nr; ++r) {
                int64_t* c = counts.data() + 256 * ((size_t)r + (size_t)nr * p);
                const uint64_t want = prefix[p + (size_t)d * r];
                for (int64_t i = 0; i < S; ++i) {
                    const uint64_t k = key[(size_t)p * S + i];
                    if (shift == 56 || (k >> (shift + 8)) == want) ++c[(k >> shift) & 255];
                }
            }
        rc = demcz_select_step(d, nr, counts.data(), prefix.data(), rank.data());
        if (rc) { std::fprintf(stderr, "demcz_select_step at shift %d: %d\n", shift, rc); return 3 + rc; }
    }
    std::vector<uint64_t> klo((size_t)d * nq), khi((size_t)d * nq);
    for (int p = 0; p < d; ++p)
        for (int j = 0; j < nq; ++j) { klo[p + (size_t)d * j] = prefix[p + (size_t)d * (2 * j)]; khi[p + (size_t)d * j] = prefix[p + (size_t)d * (2 * j + 1)]; }
    std::vector<double> q((size_t)d * nq), lower((size_t)d * nq), upper((size_t)d * nq);
    rc = demcz_quantile_finish(d, nq, klo.data(), khi.data(), frac.data(), nan.data(), q.data(), lower.data(), upper.data());
    if (rc) { std::fprintf(stderr, "demcz_quantile_finish: %d\n", rc); return 3 + rc; }
    for (int p = 0; p < d; ++p)
        for (int j = 0; j < nq; ++j) {
            uint64_t b[3];
            const double v[3] = {q[p + (size_t)d * j], lower[p + (size_t)d * j], upper[p + (size_t)d * j]};
            std::memcpy(b, v, sizeof b);
            std::printf("%016llx %016llx %016llx\n", (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2]);
        }
    return 0;
}
