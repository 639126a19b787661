// density_host_main.cpp -- the host half of the posterior densities (demc.jl_amd/csrc/demcz_density_host.h) as a stand-alone
// program, so that it can be built with -fsanitize=address,undefined and run on its own (tests/test_density_reference.py).
//
//   plan  FILE   text, one case per line: d nbx nby npairs p q p q ...  ->  "cap a b ntiles columns_read", then per tile
//                "nrow ncol npair mask(hex) | row x8 | col x8 | col_row x8 | out x npair"
//   place FILE   binary (native endianness): int64 nb, n; doubles lo, hi; n doubles  ->  the edge table's bit patterns on one
//                line, then the bin of every draw by density_bin (the text the kernels compile), one per line
//   steps FILE   text, one case per line: S prob (prob as a hexadecimal bit pattern)  ->  "status m"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../demc.jl_amd/csrc/demcz_density_host.h"

static int run_plan(std::FILE* f)
{
    int d, nbx, nby, npairs;
    while (std::fscanf(f, "%d %d %d %d", &d, &nbx, &nby, &npairs) == 4) {
        std::vector<int32_t> pairs((size_t)2 * (npairs > 0 ? npairs : 0));
        for (int32_t& v : pairs)
            if (std::fscanf(f, "%d", &v) != 1) return 2;
        demcz::DensityPlan plan;
        const int32_t rc = demcz::density_plan(d, npairs, pairs.data(), nbx, nby, plan);
        if (rc) { std::printf("refused %d\n", rc); continue; }
        std::printf("%d %d %d %zu %" PRId64 "\n", plan.cap, plan.a, plan.b, plan.tiles.size(), plan.columns_read);
        for (const demcz::DensityTile& T : plan.tiles) {
            std::printf("%d %d %d %08x%08x |", T.nrow, T.ncol, T.npair, T.mask_hi, T.mask_lo);
            for (int k = 0; k < demcz::DENSITY_TILE_SIDE; ++k) std::printf(" %d", T.row[k]);
            std::printf(" |");
            for (int k = 0; k < demcz::DENSITY_TILE_SIDE; ++k) std::printf(" %d", T.col[k]);
            std::printf(" |");
            for (int k = 0; k < demcz::DENSITY_TILE_SIDE; ++k) std::printf(" %d", T.col_row[k]);
            std::printf(" |");
            for (int k = 0; k < T.npair; ++k) std::printf(" %d", T.out[k]);
            std::printf("\n");
        }
    }
    return 0;
}

static int run_place(std::FILE* f)
{
    int64_t hdr[2];
    double range[2];
    if (std::fread(hdr, sizeof(int64_t), 2, f) != 2 || std::fread(range, sizeof(double), 2, f) != 2 || hdr[1] < 0) return 2;
    const int nb = (int)hdr[0];
    std::vector<double> x((size_t)hdr[1]), e((size_t)(nb > 0 ? nb : 0) + 1);
    if (std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) return 2;
    const int32_t rc = demcz_histogram_edges(nb, range[0], range[1], e.data());
    if (rc) { std::printf("refused %d\n", rc); return 0; }
    for (double v : e) {
        uint64_t b;
        std::memcpy(&b, &v, sizeof b);
        std::printf("%016" PRIx64 " ", b);
    }
    std::printf("\n");
    const double lo = e[0], hi = e[(size_t)nb];
    for (double v : x) std::printf("%d\n", demcz::density_bin(v, e.data(), nb, lo, hi, hi - lo));
    return 0;
}

static int run_steps(std::FILE* f)
{
    long long S;
    unsigned long long bitsofp;
    while (std::fscanf(f, "%lld %llx", &S, &bitsofp) == 2) {
        double prob;
        const uint64_t b = bitsofp;
        std::memcpy(&prob, &b, sizeof prob);
        int64_t m = -1;
        const int32_t rc = demcz_hdi_steps((int64_t)S, 1, &prob, &m);
        std::printf("%d %" PRId64 "\n", rc, m);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s plan|place|steps INPUT\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 2; }
    int rc = 2;
    if (!std::strcmp(argv[1], "plan")) rc = run_plan(f);
    else if (!std::strcmp(argv[1], "place")) rc = run_place(f);
    else if (!std::strcmp(argv[1], "steps")) rc = run_steps(f);
    std::fclose(f);
    return rc;
}
