// rank_host_main.cpp -- the rank -> normal score step (demc.jl_amd/csrc/demcz_rank_host.h) as a stand-alone program, so that it
// can be built with -fsanitize=address,undefined and run on its own (tests/test_rank_reference.py).
//
// Input file (native endianness): int64 S, n; n doubles (average ranks).  Output: one line per rank with the bit pattern of its
// normal score in hexadecimal, as demcz_rank_to_z returns it; then one line per rank formed from counts -- the rank is read back
// as (less, equal) = (r - 1, 1) for a whole r and (r - 3/2, 2) otherwise, put together again by rank_average and scored.  Exit code 3 + the status
// when demcz_rank_to_z refuses the input.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../demc.jl_amd/csrc/demcz_rank_host.h"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int64_t hdr[2];
    if (std::fread(hdr, sizeof(int64_t), 2, f) != 2 || hdr[1] < 0 || hdr[1] > (1 << 24)) { std::fclose(f); return 2; }
    const int64_t S = hdr[0], n = hdr[1];
    std::vector<double> r((size_t)n), z((size_t)n);
    if (std::fread(r.data(), sizeof(double), r.size(), f) != r.size()) { std::fclose(f); return 2; }
    std::fclose(f);
    const int32_t rc = demcz_rank_to_z(n, r.data(), S, z.data());
    if (rc) { std::fprintf(stderr, "demcz_rank_to_z: %d\n", rc); return 3 + rc; }
    for (int64_t i = 0; i < n; ++i) {
        uint64_t b;
        std::memcpy(&b, &z[(size_t)i], sizeof b);
        std::printf("%016llx\n", (unsigned long long)b);
    }
    for (int64_t i = 0; i < n; ++i) {
        const bool whole = std::floor(r[(size_t)i]) == r[(size_t)i];
        const int64_t less = (int64_t)std::floor(r[(size_t)i] - (whole ? 1.0 : 1.5));
        const int64_t equal = whole ? 1 : 2;
        const double v = demcz::rank_to_z(demcz::rank_average(less, equal), (double)S);
        uint64_t b;
        std::memcpy(&b, &v, sizeof b);
        std::printf("%016llx\n", (unsigned long long)b);
    }
    return 0;
}
