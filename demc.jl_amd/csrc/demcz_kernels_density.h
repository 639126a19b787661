// demcz_kernels_density.h -- K13: what the posterior looks like, from the resident history (gfx950; DESIGN.md sections 3 and
// 4.18): marginal histograms, pairwise histograms and the arg-min behind the highest-density interval.  Integer counts only:
// exact, independent of the order of the additions, additive over shards.
//
//   histogram_kernel     one pass over the window, the shape of select_counts_kernel: for parameter p,
//                            counts[p][k] += #{draws x of p : edges[p][k] <= x < edges[p][k+1]}   (the last bin takes x == edges[p][nb]),
//                            counts[p][nb] += #{x < edges[p][0]},  counts[p][nb+1] += #{x > edges[p][nb]},  counts[p][nb+2] += #{x != x}.
//   histogram2d_kernel   one pass per tile of pairs (demcz_density_host.h): a lane loads its draw of every parameter of the tile
//                            once, places each in its row table (nbx bins) and / or its column table (nby bins), and adds one to
//                            the cell of every requested pair of the tile whose two coordinates are in range.
//   hdi_partial_kernel / hdi_final_kernel   over the ascending keys the ranks' sort leaves: the arg-min over 0 <= i < S - m of
//                            (value(key[i + m]) - value(key[i]), i): the smaller width wins, on == the smaller i, a NaN width is
//                            never a candidate.  One partial per workgroup, one workgroup per (parameter, probability) finishes
//                            and writes the two ends (NaN, NaN without a candidate or with a NaN draw in the window).
//
// density_bin (demcz_density_host.h: one text for the device and the host) places a draw: the estimate (x - lo) / (hi - lo) * nb,
// then a walk along the table, bounded by nb steps either way, until edges[k] <= x < edges[k+1] (or k is the last bin): the table
// decides, not the rounding of the estimate.
//
// No waits between workgroups, no spin loops, no floating-point atomics.  32-bit LDS counters (a workgroup sees at most 64 chains
// x 2^20 generations: the host's chunk plan), flushed with one 64-bit global atomic per non-empty counter.
//
// Bounds: a history load is of chain c < N, parameter p < d and slot s0 + g with 0 <= g < w, under the lane's own predicate:
// inside the window check_hist_range admitted; in histogram2d_kernel p is a row or column entry of the tile below its nrow / ncol,
// which the plan took from the caller's checked pairs.  A table load is edges[p][k] or edges[p][k+1] with 0 <= k <= nb - 1 of a
// table of nb + 1 entries.  A marginal counter index is a code in 0..nb+2 of nb + 3 counters (nb <= 4096: the array holds 4099).
// A cell index is slot * nbx * nby + bx * nby + by with slot < npair <= cap, bx < nbx, by < nby: below cap nbx nby <= 16384
// counters, the dynamic LDS the launch asks for.  The hdi kernels read key[i] and key[i + m] with i + m < S, and partials at
// indices below gridDim.x.
#pragma once

#include "demcz_device.h"
#include "demcz_density_host.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int DEN_BS = 256;     // four waves: they share the 64 chains and the counters, and take the generations in turn
constexpr int DEN_U = 4;        // generations a wave of histogram_kernel loads before it counts them
constexpr int DEN_U2 = 2;       // ... of histogram2d_kernel, which loads every parameter of its tile per generation

// grid: x = parameter * cb + chain block of 64 (a workgroup stays inside one parameter), y = time chunk of `per` generations.
// edges: [d][nb + 1];  counts: [d][nb + 3].
__global__ void __launch_bounds__(DEN_BS) histogram_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t w,
                                                           int64_t cb, int64_t per, int nb, const double* __restrict__ edges,
                                                           unsigned long long* counts)
{
    __shared__ unsigned int hist[DENSITY_MAX_BINS + 3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p = blockIdx.x / cb, c = (blockIdx.x % cb) * 64 + lane;
    const bool valid = c < N;
    const int64_t nd = N * d;
    const int64_t g_lo = (int64_t)blockIdx.y * per, g_hi = (g_lo + per < w) ? g_lo + per : w;
    const int ncode = nb + 3;
    const double* e = edges + p * (nb + 1);
    const double lo = e[0], hi = e[nb], span = hi - lo;
    for (int i = tid; i < ncode; i += DEN_BS) hist[i] = 0u;
    __syncthreads();

    const double* base = chain + (valid ? c : 0) + N * p + nd * s0;
    // a run of wave-uniform hits (every counting lane of the wave in one bin: the central bins of a posterior) is kept in scalars
    // and added once when the bin changes
    int pend_code = -1;
    unsigned int pend_cnt = 0u;
    for (int64_t gb = g_lo + (int64_t)wv * DEN_U; gb < g_hi; gb += (int64_t)(DEN_BS / 64) * DEN_U) {
        double x[DEN_U];
        bool ok[DEN_U];
#pragma unroll
        for (int k = 0; k < DEN_U; ++k) {
            ok[k] = valid && gb + k < g_hi;
            x[k] = ok[k] ? base[nd * (gb + k)] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < DEN_U; ++k) {
            const int code = ok[k] ? density_bin(x[k], e, nb, lo, hi, span) : -1;
            const unsigned long long m = __ballot(code >= 0);
            if (m) {                                                     // wave-uniform
                const int first = __builtin_amdgcn_readlane(code, __ffsll(m) - 1);
                const unsigned long long same = __ballot(code == first);
                if (same == m) {                                         // wave-uniform: one bin for the whole wave
                    if (first != pend_code) {
                        if (pend_cnt && lane == 0) atomicAdd(&hist[pend_code], pend_cnt);
                        pend_code = first;
                        pend_cnt = 0u;
                    }
                    pend_cnt += (unsigned int)__popcll(m);
                } else if (code >= 0) {
                    atomicAdd(&hist[code], 1u);
                }
            }
        }
    }
    if (pend_cnt && lane == 0) atomicAdd(&hist[pend_code], pend_cnt);
    __syncthreads();
    unsigned long long* out = counts + p * ncode;
    for (int i = tid; i < ncode; i += DEN_BS) {
        const unsigned int v = hist[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
}

// grid: x = tile * cb + chain block of 64, y = time chunk of `per` generations; dynamic LDS: cap * nbx * nby counters.
// ex: [d][nbx + 1], ey: [d][nby + 1];  tiles: the plan's;  counts: [npairs][nbx][nby].
__global__ void __launch_bounds__(DEN_BS) histogram2d_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t w,
                                                             int64_t cb, int64_t per, int nbx, int nby, const double* __restrict__ ex,
                                                             const double* __restrict__ ey, const DensityTile* __restrict__ tiles,
                                                             unsigned long long* counts)
{
    extern __shared__ unsigned int cells[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const DensityTile& T = tiles[blockIdx.x / cb];
    const int64_t c = (blockIdx.x % cb) * 64 + lane;
    const bool valid = c < N;
    const int64_t nd = N * d;
    const int64_t g_lo = (int64_t)blockIdx.y * per, g_hi = (g_lo + per < w) ? g_lo + per : w;
    const int ncell = nbx * nby, nrow = T.nrow, ncol = T.ncol, total = T.npair * ncell;
    const unsigned long long mask = ((unsigned long long)T.mask_hi << 32) | T.mask_lo;
    for (int i = tid; i < total; i += DEN_BS) cells[i] = 0u;
    __syncthreads();

    const double* base = chain + (valid ? c : 0) + nd * s0;
    for (int64_t gb = g_lo + (int64_t)wv * DEN_U2; gb < g_hi; gb += (int64_t)(DEN_BS / 64) * DEN_U2) {
        double xr[DEN_U2][DENSITY_TILE_SIDE], xc[DEN_U2][DENSITY_TILE_SIDE];
        bool ok[DEN_U2];
#pragma unroll
        for (int k = 0; k < DEN_U2; ++k) {
            ok[k] = valid && gb + k < g_hi;
#pragma unroll
            for (int r = 0; r < DENSITY_TILE_SIDE; ++r) {
                xr[k][r] = (ok[k] && r < nrow) ? base[N * T.row[r] + nd * (gb + k)] : 0.0;
                xc[k][r] = (ok[k] && r < ncol && T.col_row[r] < 0) ? base[N * T.col[r] + nd * (gb + k)] : 0.0;
            }
        }
#pragma unroll
        for (int k = 0; k < DEN_U2; ++k) {
            int bx[DENSITY_TILE_SIDE], by[DENSITY_TILE_SIDE];
#pragma unroll
            for (int r = 0; r < DENSITY_TILE_SIDE; ++r) {
                bx[r] = -1;
                if (r < nrow) {                                          // wave-uniform
                    const double* e = ex + (int64_t)T.row[r] * (nbx + 1);
                    const double lo = e[0], hi = e[nbx];
                    const int b = density_bin(xr[k][r], e, nbx, lo, hi, hi - lo);
                    bx[r] = (ok[k] && b < nbx) ? b : -1;
                }
            }
#pragma unroll
            for (int cc = 0; cc < DENSITY_TILE_SIDE; ++cc) {
                by[cc] = -1;
                if (cc < ncol) {                                         // wave-uniform
                    double y = xc[k][cc];
                    const int from = T.col_row[cc];
#pragma unroll
                    for (int r = 0; r < DENSITY_TILE_SIDE; ++r) y = (from == r) ? xr[k][r] : y;
                    const double* e = ey + (int64_t)T.col[cc] * (nby + 1);
                    const double lo = e[0], hi = e[nby];
                    const int b = density_bin(y, e, nby, lo, hi, hi - lo);
                    by[cc] = (ok[k] && b < nby) ? b : -1;
                }
            }
#pragma unroll
            for (int r = 0; r < DENSITY_TILE_SIDE; ++r)
#pragma unroll
                for (int cc = 0; cc < DENSITY_TILE_SIDE; ++cc) {
                    const int bit = r * DENSITY_TILE_SIDE + cc;
                    if ((mask >> bit) & 1ull) {                          // wave-uniform
                        const int slot = __popcll(mask & ((1ull << bit) - 1ull));
                        if (bx[r] >= 0 && by[cc] >= 0) atomicAdd(&cells[slot * ncell + bx[r] * nby + by[cc]], 1u);
                    }
                }
        }
    }
    __syncthreads();
    for (int i = tid; i < total; i += DEN_BS) {
        const unsigned int v = cells[i];
        if (v) {
            const int slot = i / ncell;
            atomicAdd(&counts[(int64_t)T.out[slot] * ncell + (i - slot * ncell)], (unsigned long long)v);
        }
    }
}

// ---- the highest-density interval over sorted keys ------------------------------------------------------------------------------
struct HdiSteps { long long m[DENSITY_MAX_PROBS]; };

// the double whose order-preserving key (sel_key) is k
__device__ __forceinline__ double hdi_value_of(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k ^ (1ull << 63)) : ~k;
    return __longlong_as_double((long long)b);
}

// a beats b
__device__ __forceinline__ bool hdi_beats(double aw, long long ai, double bw, long long bi)
{
    return ai >= 0 && (bi < 0 || aw < bw || (aw == bw && ai < bi));
}

__device__ __forceinline__ void hdi_block_reduce(double& v, long long& i, double* rv, long long* ri)
{
    rv[threadIdx.x] = v;
    ri[threadIdx.x] = i;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && hdi_beats(rv[threadIdx.x + s], ri[threadIdx.x + s], rv[threadIdx.x], ri[threadIdx.x])) {
            rv[threadIdx.x] = rv[threadIdx.x + s];
            ri[threadIdx.x] = ri[threadIdx.x + s];
        }
        __syncthreads();
    }
    v = rv[0];
    i = ri[0];
}

// grid: x = partial, y = probability, z = parameter.  where[p]: the buffer that holds parameter p's sorted keys.
// pv / pi: [d][nprob][gridDim.x].
__global__ void __launch_bounds__(256) hdi_partial_kernel(const uint64_t* __restrict__ buf0, const uint64_t* __restrict__ buf1,
                                                          const int* __restrict__ where, int64_t S, HdiSteps steps, double* pv, long long* pi)
{
    __shared__ double rv[256];
    __shared__ long long ri[256];
    const int64_t p = blockIdx.z, j = blockIdx.y;
    const int64_t m = steps.m[j], ncand = S - m;
    const uint64_t* sorted = (where[p] ? buf1 : buf0) + p * S;
    double bw = __longlong_as_double(0x7ff8000000000000ll);
    long long bi = -1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ncand; i += (int64_t)gridDim.x * 256) {
        const double hi = hdi_value_of(sorted[i + m]), lo = hdi_value_of(sorted[i]);
        const double width = hi - lo;
        if (width == width && hdi_beats(width, i, bw, bi)) { bw = width; bi = i; }
    }
    hdi_block_reduce(bw, bi, rv, ri);
    if (threadIdx.x == 0) {
        const int64_t at = (p * gridDim.y + j) * gridDim.x + blockIdx.x;
        pv[at] = bw;
        pi[at] = bi;
    }
}

// grid: x = probability, y = parameter; nb partials each.  out: [d][nprob][2].
__global__ void __launch_bounds__(256) hdi_final_kernel(const uint64_t* __restrict__ buf0, const uint64_t* __restrict__ buf1,
                                                        const int* __restrict__ where, const unsigned long long* __restrict__ nan_count,
                                                        int64_t S, HdiSteps steps, const double* pv, const long long* pi, int nb, double* out)
{
    __shared__ double rv[256];
    __shared__ long long ri[256];
    const int64_t p = blockIdx.y, j = blockIdx.x;
    const int64_t at = (p * gridDim.x + j) * nb;
    double bw = __longlong_as_double(0x7ff8000000000000ll);
    long long bi = -1;
    for (int k = threadIdx.x; k < nb; k += 256)
        if (hdi_beats(pv[at + k], pi[at + k], bw, bi)) { bw = pv[at + k]; bi = pi[at + k]; }
    hdi_block_reduce(bw, bi, rv, ri);
    if (threadIdx.x == 0) {
        const uint64_t* sorted = (where[p] ? buf1 : buf0) + p * S;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const bool none = bi < 0 || nan_count[p] != 0ull;
        double* o = out + (p * gridDim.x + j) * 2;
        o[0] = none ? nan : hdi_value_of(sorted[bi]);                    // (bi + m < S: bi was a candidate)
        o[1] = none ? nan : hdi_value_of(sorted[bi + steps.m[j]]);
    }
}

}  // namespace demcz
