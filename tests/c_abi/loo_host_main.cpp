// loo_host_main.cpp -- the host half of PSIS-LOO (demc.jl_amd/csrc/demcz_loo_host.h) as a stand-alone program, so that it can be
// built with -fsanitize=address,undefined and run on its own (tests/test_loo_plan.py).
//
//   loo_host_main plan FILE   FILE: lines "nobs S budget".  Per line: "case mc nchunks", then one line "from count" per chunk as
//                             loo_chunk gives them, and one more for the chunk past the end.
//   loo_host_main tail FILE   FILE: lines "S r_eff".  Per line: the status of demcz_psis_tail_length and M.
//   loo_host_main fit FILE    FILE (native endianness): int64 n, then n doubles ascending.  Prints the status of demcz_gpd_fit and
//                             the bit patterns of k, sigma and khat, then the smoothed log weights of positions 1, n/2 and n.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../demc.jl_amd/csrc/demcz_loo_host.h"

static unsigned long long bits(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s plan|tail|fit FILE\n", argv[0]); return 2; }
    const bool fit = std::strcmp(argv[1], "fit") == 0;
    std::FILE* f = std::fopen(argv[2], fit ? "rb" : "r");
    if (!f) { std::perror(argv[2]); return 2; }
    if (std::strcmp(argv[1], "plan") == 0) {
        long long nobs, S, budget;
        while (std::fscanf(f, "%lld %lld %lld", &nobs, &S, &budget) == 3) {
            const int mc = demcz::loo_chunk_width(S, budget);
            const int64_t nchunks = demcz::loo_chunk_count(nobs, mc);
            std::printf("case %d %lld\n", mc, (long long)nchunks);
            std::vector<char> seen((size_t)(nobs > 0 ? nobs : 0), 0);
            for (int64_t i = 0; i <= nchunks; ++i) {
                int64_t from = -1;
                int count = -1;
                demcz::loo_chunk(nobs, mc, i, &from, &count);
                for (int k = 0; k < count; ++k) seen[(size_t)(from + k)] += 1;       // (out of range: the sanitizer says so)
                std::printf("%lld %d\n", (long long)from, count);
            }
            for (char c : seen) if (c != 1) { std::fprintf(stderr, "an observation is not covered exactly once\n"); return 4; }
        }
    } else if (std::strcmp(argv[1], "tail") == 0) {
        long long S;
        double r;
        while (std::fscanf(f, "%lld %lf", &S, &r) == 2) {
            int64_t M = -1;
            const int32_t rc = demcz_psis_tail_length(S, r, &M);
            std::printf("%d %lld\n", rc, (long long)M);
        }
    } else if (fit) {
        int64_t n = 0;
        if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1 << 20)) { std::fclose(f); return 2; }
        std::vector<double> x((size_t)n);
        if (std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) { std::fclose(f); return 2; }
        double k = 0.0, sigma = 0.0, khat = 0.0;
        const int32_t rc = demcz_gpd_fit(n, x.data(), &k, &sigma, &khat);
        std::printf("%d %016llx %016llx %016llx\n", rc, bits(k), bits(sigma), bits(khat));
        if (rc == 0)
            for (int64_t j : {(int64_t)1, n / 2, n})
                std::printf("%016llx\n", bits(demcz::psis_smoothed(j, n, k, sigma, 0.25)));
    } else {
        std::fclose(f);
        return 2;
    }
    std::fclose(f);
    return 0;
}
