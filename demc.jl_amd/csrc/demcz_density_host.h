// demcz_density_host.h -- the host half of the posterior densities (DESIGN.md sections 3 and 4.18): the edge table of a uniform
// histogram, the number of steps of a highest-density interval and the pair-tile plan of demcz_histogram2d.  Plain C++, no HIP
// calls, so that it also builds into a stand-alone program (tests/c_abi/density_host_main.cpp).
//
// The edge table is numpy.linspace(lo, hi, nbins + 1) restated: with delta = hi - lo and step = delta / nbins,
//   edges[k] = k * step + lo            (two rounded operations, no fma)            when step != 0,
//   edges[k] = (k / nbins) * delta + lo                                             when step == 0 (delta / nbins underflowed),
//   edges[nbins] = hi.
// The table is non-decreasing (demcz_histogram_edges refuses the subnormal spans where it would not be).  The kernels (demcz_kernels_density.h) place a draw by the table alone (density_bin, below).
//
// The pair-tile plan: a tile is a set of at most DENSITY_TILE_SIDE row parameters times a set of at most DENSITY_TILE_SIDE
// column parameters; it holds the requested pairs (p, q) with p among its rows and q among its columns, at most `cap` of them,
// cap = DENSITY_LDS_CELLS / (nbx nby): their 32-bit counters fit in 64 KB of LDS together.  A workgroup of the tile reads every
// parameter of the tile once, whatever the number of its pairs.  The distinct row parameters, ascending, are cut into groups of
// a, the distinct column parameters into groups of b, a b <= cap; every (row group, column group) that holds a requested pair
// is a tile.  So every requested pair lies in exactly one tile.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/demcz.h"

#if defined(__HIPCC__)
#define DEMCZ_DENSITY_HD __host__ __device__
#else
#define DEMCZ_DENSITY_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace demcz {

constexpr int DENSITY_MAX_BINS = 4096;                // marginal histogram: 16 KB of 32-bit LDS counters (and three more)
constexpr int DENSITY_MAX_SIDE = 128;                 // pair grid: 128 x 128 cells are the 64 KB of one pair
constexpr int DENSITY_LDS_CELLS = 16384;              // 64 KB of 32-bit counters: the most LDS one workgroup may have
constexpr int DENSITY_TILE_SIDE = 8;                  // row parameters, and column parameters, of a tile at the most
constexpr int DENSITY_TILE_PAIRS = DENSITY_TILE_SIDE * DENSITY_TILE_SIDE;
constexpr int DENSITY_MAX_PROBS = 16;                 // probabilities of one demcz_hdi call

// The bin of x in the table e[0..nb], one text for the kernels and the host: 0..nb-1, or nb (below), nb + 1 (above), nb + 2 (NaN).
// lo = e[0], hi = e[nb], span = hi - lo.  The estimate (x - lo) / span * nb, then a walk along the table, bounded by nb steps
// either way, until e[k] <= x < e[k+1] (or k is the last bin).  Reads e[k] and e[k+1] with 0 <= k <= nb - 1 only.
DEMCZ_DENSITY_HD inline int density_bin(double x, const double* e, int nb, double lo, double hi, double span)
{
    const bool in = x >= lo && x <= hi;                                  // (false for a NaN; -0.0 compares as 0.0)
    int k = 0;
    if (in) {
        const double t = (x - lo) / span * (double)nb;                   // in [0, nb] up to its rounding
        k = (int)t;
        k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
        for (int i = 0; i < nb && k > 0 && x < e[k]; ++i) --k;
        for (int i = 0; i < nb && k < nb - 1 && x >= e[k + 1]; ++i) ++k;
    }
    return in ? k : (x != x ? nb + 2 : (x < lo ? nb : nb + 1));
}

// What a workgroup of a tile needs, as the kernel reads it (32-bit words throughout).
// bit r * DENSITY_TILE_SIDE + c of mask: the pair (row[r], col[c]) is requested; its counters are the tile's slot number
// popcount(mask below that bit), and out[slot] is the pair's place in the caller's (deduplicated) list.
struct DensityTile {
    int32_t nrow, ncol, npair, pad;
    uint32_t mask_lo, mask_hi;
    int32_t row[DENSITY_TILE_SIDE];
    int32_t col[DENSITY_TILE_SIDE];
    int32_t col_row[DENSITY_TILE_SIDE];               // the row slot that holds column c's parameter too, or -1: it is loaded once
    int32_t out[DENSITY_TILE_PAIRS];
};

struct DensityPlan {
    int cap = 0, a = 0, b = 0;                        // pairs per tile at the most; rows and columns per group
    std::vector<DensityTile> tiles;
    int64_t columns_read = 0;                         // sum over the tiles of their distinct parameters: a call reads 8 S of these bytes
};

// pairs: npairs distinct (p, q), p != q, both in 0..d-1 (the caller has checked).  1 <= nbx, nby <= DENSITY_MAX_SIDE.
inline int32_t density_plan(int32_t d, int32_t npairs, const int32_t* pairs, int32_t nbx, int32_t nby, DensityPlan& plan)
{
    if (d < 1 || npairs < 1 || !pairs || nbx < 1 || nby < 1 || nbx > DENSITY_MAX_SIDE || nby > DENSITY_MAX_SIDE)
        return DEMCZ_ERR_INVALID_ARGUMENT;
    plan.cap = std::min(DENSITY_TILE_PAIRS, DENSITY_LDS_CELLS / (nbx * nby));
    int a = 1;
    while ((a + 1) * (a + 1) <= plan.cap && a + 1 <= DENSITY_TILE_SIDE) ++a;
    plan.a = a;
    plan.b = std::min(DENSITY_TILE_SIDE, plan.cap / a);
    // group of a parameter in its role: -1 when it has none
    std::vector<int> rgroup((size_t)d, -1), cgroup((size_t)d, -1), rslot((size_t)d, 0), cslot((size_t)d, 0);
    std::vector<char> isrow((size_t)d, 0), iscol((size_t)d, 0);
    for (int i = 0; i < npairs; ++i) { isrow[pairs[2 * i]] = 1; iscol[pairs[2 * i + 1]] = 1; }
    int nr = 0, nc = 0;
    for (int p = 0; p < d; ++p) {
        if (isrow[p]) { rgroup[p] = nr / plan.a; rslot[p] = nr % plan.a; ++nr; }
        if (iscol[p]) { cgroup[p] = nc / plan.b; cslot[p] = nc % plan.b; ++nc; }
    }
    const int ngr = (nr + plan.a - 1) / plan.a, ngc = (nc + plan.b - 1) / plan.b;
    std::vector<int> tile_of((size_t)ngr * ngc, -1);
    plan.tiles.clear();
    // pass 1: the tiles and their parameters; pass 2 (below) numbers the slots in bit order
    for (int i = 0; i < npairs; ++i) {
        const int p = pairs[2 * i], q = pairs[2 * i + 1];
        int& t = tile_of[(size_t)rgroup[p] * ngc + cgroup[q]];
        if (t < 0) {
            t = (int)plan.tiles.size();
            DensityTile nt = {};
            for (int k = 0; k < DENSITY_TILE_SIDE; ++k) nt.row[k] = nt.col[k] = -1;
            for (int k = 0; k < DENSITY_TILE_PAIRS; ++k) nt.out[k] = -1;
            plan.tiles.push_back(nt);
        }
        DensityTile& T = plan.tiles[(size_t)t];
        T.row[rslot[p]] = p;
        T.col[cslot[q]] = q;
        const int bit = rslot[p] * DENSITY_TILE_SIDE + cslot[q];
        if (bit < 32) T.mask_lo |= 1u << bit; else T.mask_hi |= 1u << (bit - 32);
    }
    // the rows and columns a tile uses are packed to the front (slots of a group that no pair of this tile uses are dropped)
    for (DensityTile& T : plan.tiles) {
        int rmap[DENSITY_TILE_SIDE], cmap[DENSITY_TILE_SIDE], row[DENSITY_TILE_SIDE], col[DENSITY_TILE_SIDE];
        int n = 0;
        for (int k = 0; k < DENSITY_TILE_SIDE; ++k) { rmap[k] = -1; if (T.row[k] >= 0) { row[n] = T.row[k]; rmap[k] = n++; } }
        T.nrow = n;
        for (int k = 0; k < DENSITY_TILE_SIDE; ++k) T.row[k] = (k < n) ? row[k] : -1;
        n = 0;
        for (int k = 0; k < DENSITY_TILE_SIDE; ++k) { cmap[k] = -1; if (T.col[k] >= 0) { col[n] = T.col[k]; cmap[k] = n++; } }
        T.ncol = n;
        for (int k = 0; k < DENSITY_TILE_SIDE; ++k) T.col[k] = (k < n) ? col[k] : -1;
        const uint64_t old = ((uint64_t)T.mask_hi << 32) | T.mask_lo;
        uint64_t m = 0;
        for (int bit = 0; bit < DENSITY_TILE_PAIRS; ++bit)
            if ((old >> bit) & 1) m |= (uint64_t)1 << (rmap[bit / DENSITY_TILE_SIDE] * DENSITY_TILE_SIDE + cmap[bit % DENSITY_TILE_SIDE]);
        T.mask_lo = (uint32_t)m;
        T.mask_hi = (uint32_t)(m >> 32);
    }
    for (int i = 0; i < npairs; ++i) {
        const int p = pairs[2 * i], q = pairs[2 * i + 1];
        DensityTile& T = plan.tiles[(size_t)tile_of[(size_t)rgroup[p] * ngc + cgroup[q]]];
        int r = 0, c = 0;
        while (T.row[r] != p) ++r;
        while (T.col[c] != q) ++c;
        const int bit = r * DENSITY_TILE_SIDE + c;
        const uint64_t m = ((uint64_t)T.mask_hi << 32) | T.mask_lo;
        const uint64_t below = m & (((uint64_t)1 << bit) - 1);
        int slot = 0;
        for (uint64_t v = below; v; v &= v - 1) ++slot;
        T.out[slot] = i;
    }
    plan.columns_read = 0;
    for (DensityTile& T : plan.tiles) {
        const uint64_t m = ((uint64_t)T.mask_hi << 32) | T.mask_lo;
        int np = 0;
        for (uint64_t v = m; v; v &= v - 1) ++np;
        T.npair = np;
        int distinct = T.nrow;
        for (int c = 0; c < DENSITY_TILE_SIDE; ++c) {
            T.col_row[c] = -1;
            if (c >= T.ncol) continue;
            for (int r = 0; r < T.nrow; ++r)
                if (T.row[r] == T.col[c]) T.col_row[c] = r;
            distinct += T.col_row[c] < 0 ? 1 : 0;
        }
        plan.columns_read += distinct;
    }
    return DEMCZ_OK;
}

}  // namespace demcz

// numpy.linspace(lo, hi, nbins + 1) into edges[0..nbins].  lo < hi, both finite, hi - lo finite, 1 <= nbins <= 4096, and the
// table non-decreasing.
extern "C" int32_t demcz_histogram_edges(int32_t nbins, double lo, double hi, double* edges)
{
    if (!edges || nbins < 1 || nbins > demcz::DENSITY_MAX_BINS) return DEMCZ_ERR_INVALID_ARGUMENT;
    const double delta = hi - lo;
    if (!(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(delta)) return DEMCZ_ERR_INVALID_ARGUMENT;
    const double div = (double)nbins;
    const double step = delta / div;
    for (int k = 0; k <= nbins; ++k) {
        double y;
        if (step != 0.0) {
            const double t = (double)k * step;
            y = t + lo;
        } else {
            const double f = (double)k / div;
            const double t = f * delta;
            y = t + lo;
        }
        edges[k] = y;
    }
    edges[nbins] = hi;
    // between normal doubles the table cannot decrease (k <= nbins - 1 < nbins leaves room for its three roundings); a span of a
    // few thousand subnormals, whose step rounds absolutely, can: such a table places nothing and is refused
    for (int k = 0; k < nbins; ++k)
        if (edges[k] > edges[k + 1]) return DEMCZ_ERR_INVALID_ARGUMENT;
    return DEMCZ_OK;
}

// m = min(floor(prob S), S - 1): the steps a highest-density interval of probability prob spans among S sorted draws.
extern "C" int32_t demcz_hdi_steps(int64_t S, int32_t nprob, const double* probs, int64_t* steps)
{
    if (S < 1 || nprob < 1 || nprob > demcz::DENSITY_MAX_PROBS || !probs || !steps) return DEMCZ_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < nprob; ++j)
        if (!(probs[j] > 0.0 && probs[j] < 1.0)) return DEMCZ_ERR_INVALID_ARGUMENT;            // (a NaN fails both comparisons)
    for (int j = 0; j < nprob; ++j) {
        const double v = std::floor(probs[j] * (double)S);
        int64_t m = (v < (double)S) ? (int64_t)v : S - 1;
        if (m > S - 1) m = S - 1;
        steps[j] = m < 0 ? 0 : m;
    }
    return DEMCZ_OK;
}
