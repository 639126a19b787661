// demcz_kernels_loo.h -- K11: PSIS-LOO and WAIC of the columns of a history (gfx950; DESIGN.md sections 3 and 4.16).  Column p
// holds the pointwise log-likelihoods a of observation p over the window's S = N w draws.  The keys-only radix sort of
// demcz_kernels_rank.h leaves the column's keys ascending, a_0 <= a_1 <= ..., in one of the two key buffers (where[p]); the
// importance ratios are r = -a, so the tail of the largest ratios is the FRONT of the sorted column.  The other key buffer of the
// column is free by then and takes the tail's exceedances.  All columns go through the same three launches.
//
//   psis_fit_kernel    one 256-lane workgroup per column: tail length by bisection, exceedances, the m candidate fits of
//                      demcz_loo_host.h, their weights, k, sigma and khat                                        -> fit[p]
//   loo_sum_kernel     grid (tiles of LOO_TILE sorted keys, columns): five partial sums per tile, the tail's weights
//                      recomputed from fit[p] and the element's position                                         -> part[p][tile][5]
//   loo_finish_kernel  one lane per column: the tiles added in tile order, the five outputs
//
// Every sum is a lane-strided partial, the butterfly of loo_wave_sum, and the four waves added in order through LDS: no
// floating-point atomics, a result is the same bits run to run and does not depend on the number of columns.
//
// Bounds: a load of the sorted column is sorted[i] with i = 0, S / 2, S - 1, M <= S - 1 (psis_tail_cap), a bisection midpoint
// lo <= mid < hi <= M, a tail position j < n <= M, or a tile position under the lane's own predicate i < S.  The exceedances are
// stored to and loaded from xs[i] with i < n <= M < S words of the column's other key buffer.  Candidate tables are indexed by
// j < m <= LOO_MAX_CAND (m is clamped).  part is indexed [p < columns][tile < ntiles][5], the outputs by p < columns.
#pragma once

#include "demcz_device.h"
#include "demcz_kernels_sel.h"
#include "demcz_loo_host.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int LOO_BS = 256;                         // four waves
constexpr int LOO_KPT = 4;                          // sorted keys per lane and tile
constexpr int LOO_TILE = LOO_BS * LOO_KPT;
constexpr int LOO_NPART = 5;

// what psis_fit_kernel leaves per column
struct LooFit {
    double a0, amax, shift;         // the smallest and the largest entry, and the middle one: the shift of the variance's sums
    double cutoff, expc;            // c and exp(c)
    double k, sigma, khat;
    long long n;                    // tail length
    int bad;                        // a NaN or an infinite entry: every output NaN
    int smooth;                     // the tail's weights are replaced (n >= 5 and k finite)
};

// the double behind a key of sel_key
__device__ __forceinline__ double loo_value_of(uint64_t key)
{
    const uint64_t b = (key >> 63) ? (key ^ (1ull << 63)) : ~key;
    return __longlong_as_double((long long)b);
}

// every lane gets the same sum: v[l] + v[l ^ 32], then ^ 16, ... ^ 1
__device__ __forceinline__ double loo_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum over the workgroup's 256 lanes, the same in every lane; red: 4 doubles of LDS
__device__ __forceinline__ double loo_block_sum(double v, double* red)
{
    v = loo_wave_sum(v);
    __syncthreads();                                                     // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid: x = column.  buf0 / buf1: [columns][S] keys; where[p]: the buffer with column p's sorted keys.  r_eff: columns values or null.
__global__ void __launch_bounds__(LOO_BS) psis_fit_kernel(uint64_t* buf0, uint64_t* buf1, const int* __restrict__ where,
                                                         const unsigned long long* __restrict__ nan_count,
                                                         const double* __restrict__ r_eff, int64_t S, LooFit* __restrict__ fit)
{
    __shared__ double red[LOO_BS / 64];
    __shared__ double cb[LOO_MAX_CAND], cL[LOO_MAX_CAND], cw[LOO_MAX_CAND];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int wh = where[p];
    const uint64_t* sorted = (wh ? buf1 : buf0) + p * S;
    double* xs = reinterpret_cast<double*>((wh ? buf0 : buf1) + p * S);
    LooFit f;
    f.a0 = loo_value_of(sorted[0]);
    f.amax = loo_value_of(sorted[S - 1]);
    f.shift = loo_value_of(sorted[S / 2]);
    f.cutoff = f.expc = f.k = f.sigma = __builtin_nan("");
    f.khat = __builtin_inf();
    f.n = 0;
    f.smooth = 0;
    f.bad = (nan_count[p] != 0ull || !(f.a0 > -__builtin_inf()) || !(f.amax < __builtin_inf())) ? 1 : 0;
    if (f.bad) {                                                         // uniform over the workgroup
        if (tid == 0) fit[p] = f;
        return;
    }
    const int64_t M = psis_tail_cap(S, r_eff ? r_eff[p] : 1.0);
    const uint64_t keyM = sorted[M];
    const double lwM = f.a0 - loo_value_of(keyM);
    const bool floor_cut = !(lwM > LOO_LOG_DBL_MIN);
    const double c = floor_cut ? LOO_LOG_DBL_MIN : lwM;
    // first j with lw_j <= c, in [0, M] (lw_M <= c).  Where c is lw_M that is the first j with a_j >= a_M, decided on the keys:
    // the subtraction a_0 - a_j may round two different a to one lw, and must not move the tail's end.
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t km = sorted[mid];
        const bool in_tail = floor_cut ? (f.a0 - loo_value_of(km) > c) : (km < keyM);
        if (in_tail) lo = mid + 1; else hi = mid;
    }
    const int64_t n = lo;
    f.cutoff = c;
    f.expc = exp(c);
    f.n = n;
    if (n < LOO_MIN_FIT) {
        if (tid == 0) fit[p] = f;
        return;
    }
    for (int64_t i = tid; i < n; i += LOO_BS) xs[i] = exp(f.a0 - loo_value_of(sorted[n - 1 - i])) - f.expc;
    __syncthreads();
    const double xn = xs[n - 1], xq = xs[psis_quartile(n) - 1];
    int m = psis_candidates(n);
    if (m > LOO_MAX_CAND) m = LOO_MAX_CAND;
    for (int j = 1; j <= m; ++j) {
        const double b = gpd_b(j, m, xn, xq);
        double part = 0.0;
        for (int64_t i = tid; i < n; i += LOO_BS) part += gpd_term(b, xs[i]);
        const double kj = loo_block_sum(part, red) / (double)n;
        if (tid == 0) {
            cb[j - 1] = b;
            cL[j - 1] = gpd_profile(n, b, kj);
        }
    }
    __syncthreads();
    for (int j = tid; j < m; j += LOO_BS) {
        double s = 0.0;
        for (int l = 0; l < m; ++l) s += exp(cL[l] - cL[j]);
        cw[j] = 1.0 / s;
    }
    __syncthreads();
    double bhat = 0.0;
    for (int j = 0; j < m; ++j) bhat += cb[j] * cw[j];                   // (every lane: the same additions in the same order)
    double part = 0.0;
    for (int64_t i = tid; i < n; i += LOO_BS) part += gpd_term(bhat, xs[i]);
    const double k = loo_block_sum(part, red) / (double)n;
    if (k - k == 0.0) {                                                  // finite
        f.k = k;
        f.sigma = -(k / bhat);
        f.khat = gpd_khat(n, k);
        f.smooth = 1;
    }
    if (tid == 0) fit[p] = f;
}

// grid: x = tile, y = column.  part: [columns][ntiles][LOO_NPART] =
//   sum exp(lw'), sum exp(lw' + (a - a0)), sum exp(a - amax), sum (a - shift), sum (a - shift)^2
// elpd_loo's numerator is shifted by a0: an unsmoothed term is then exp((a0 - a) + (a - a0)) = exp(0) exactly, however wide the
// column, and a tail term has a - a0 < 708 and lw' <= 0; lppd's sum is shifted by amax, the usual logsumexp.
__global__ void __launch_bounds__(LOO_BS) loo_sum_kernel(const uint64_t* __restrict__ buf0, const uint64_t* __restrict__ buf1,
                                                        const int* __restrict__ where, const LooFit* __restrict__ fit, int64_t S,
                                                        int64_t ntiles, double* __restrict__ part)
{
    __shared__ double red[LOO_BS / 64];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.y;
    const LooFit f = fit[p];
    if (f.bad) return;                                                   // uniform over the workgroup
    const uint64_t* sorted = (where[p] ? buf1 : buf0) + p * S;
    double s[LOO_NPART] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < LOO_KPT; ++kk) {
        const int64_t i = (int64_t)blockIdx.x * LOO_TILE + kk * LOO_BS + tid;
        if (i < S) {
            const double a = loo_value_of(sorted[i]);
            double lw = f.a0 - a;
            if (f.smooth && i < f.n) lw = psis_smoothed(f.n - i, f.n, f.k, f.sigma, f.expc);
            const double d0 = a - f.a0, da = a - f.amax, dv = a - f.shift;
            s[0] += exp(lw);
            s[1] += exp(lw + d0);
            s[2] += exp(da);
            s[3] += dv;
            s[4] += dv * dv;
        }
    }
    double* out = part + (p * ntiles + blockIdx.x) * LOO_NPART;
#pragma unroll
    for (int q = 0; q < LOO_NPART; ++q) {
        const double v = loo_block_sum(s[q], red);
        if (tid == 0) out[q] = v;
    }
}

// one lane per column.  out: [4][columns] = elpd_loo, pareto_k, lppd, p_waic;  n_tail: [columns]
__global__ void __launch_bounds__(64) loo_finish_kernel(const LooFit* __restrict__ fit, const double* __restrict__ part, int64_t S,
                                                       int64_t ntiles, int columns, double* __restrict__ out,
                                                       long long* __restrict__ n_tail)
{
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= columns) return;
    const LooFit f = fit[p];
    double elpd = __builtin_nan(""), khat = elpd, lppd = elpd, pw = elpd;
    if (!f.bad) {
        double s[LOO_NPART] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t t = 0; t < ntiles; ++t)
#pragma unroll
            for (int q = 0; q < LOO_NPART; ++q) s[q] += part[(p * ntiles + t) * LOO_NPART + q];
        const double dS = (double)S;
        elpd = f.a0 + (log(s[1]) - log(s[0]));
        lppd = f.amax + (log(s[2]) - log(dS));
        khat = f.khat;
        if (S > 1) {
            const double v = (s[4] - (s[3] * s[3]) / dS) / (dS - 1.0);
            pw = v > 0.0 ? v : 0.0;
        }
    }
    out[p] = elpd;
    out[(int64_t)columns + p] = khat;
    out[2 * (int64_t)columns + p] = lppd;
    out[3 * (int64_t)columns + p] = pw;
    n_tail[p] = f.bad ? 0ll : f.n;
}

}  // namespace demcz
