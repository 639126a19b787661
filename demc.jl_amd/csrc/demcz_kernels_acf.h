// demcz_kernels_acf.h -- K8: lagged self-products of the split chains over the resident history (gfx950), the device
// half of the effective sample size (BDA3 section 11.5 / the Stan reference manual, without rank normalisation; DESIGN.md
// section 3).  Window of w generations from history slot s0, n = floor(w/2); split chain (h, c) covers slots
// s0 + h n .. s0 + h n + n - 1, as in K5 (demcz_kernels.h), and is centred by its own mean_j (rhat_chainstats_kernel).
//
//   acf_products_kernel: for one lag tile [t0, t0 + ACF_TL), one half, one time chunk and one lane per (chain, parameter):
//       part[k] = sum over the chunk's left samples i of y_i * y_{i + t0 + k},   y = x - mean_j,   i + t0 + k <= n - 1.
//   acf_reduce_kernel: one workgroup per (parameter, lag): a split chain's chunk partials are added in chunk order, the split
//       chains by the fixed-order tree of rhat_reduce_kernel -> sums[p + d (t - lag_from)] = sum_j n c_j(t).
//
// Nothing here depends on which lags a launch was asked for: lag t of chain j is always the same chain of fma in generation
// order within the same chunks (the chunk plan is a function of (N, d, n) alone), so a lag costs the same bits whichever
// batch or tile origin computed it.  No floating-point atomics.
#pragma once

#include "demcz_device.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int ACF_TL = 32;      // lags per tile: 32 accumulators + a 32-sample window per lane, all in VGPRs
constexpr int ACF_U = 8;        // generations loaded ahead of their products (two loads each): 16 loads in flight per lane
constexpr int ACF_BS = 64;      // one wave per workgroup, lane = chain: small N spreads over as many SIMDs as there are waves

// grid: x over N*d in waves (chain fastest), y = h * nchunk + chunk, z = lag tile of this launch (lag t0 = lag0 + ACF_TL z)
// part: [z][y][k < ACF_TL][N*d]
//
// Bounds: every load is of slot s0 + h n + min(i, n - 1) with i >= 0, for a lane below N*d: inside the window that
// check_hist_range admitted.  A sample past the half's end is never used -- its place in a product is taken by 0.0 -- and never
// read: the clamped index reads the half's last sample instead, so that the loads need no branch and stay in flight together.
__global__ void __launch_bounds__(ACF_BS) acf_products_kernel(const double* chain, const double* mean_j, int64_t N, int d, int64_t s0,
                                                              int64_t n, int nchunk, int64_t per, int64_t lag0, double* part)
{
    const int64_t nd = N * d;
    const int64_t lane = (int64_t)blockIdx.x * ACF_BS + threadIdx.x;
    if (lane >= nd) return;
    const int h = blockIdx.y / nchunk, ck = blockIdx.y % nchunk;
    const int64_t t0 = lag0 + (int64_t)ACF_TL * blockIdx.z;
    const int64_t c0 = ck * per, c1 = (c0 + per < n) ? c0 + per : n;      // left samples of this chunk
    const int64_t last = n - 1;
    const double* base = chain + lane + nd * (s0 + h * n);
    const double mj = mean_j[lane + nd * h];

    double acc[ACF_TL], win[ACF_TL];
#pragma unroll
    for (int k = 0; k < ACF_TL; ++k) acc[k] = 0.0;
    if (t0 <= last) {                    // (a tile wholly past the last lag has nothing to add: uniform over the workgroup)
        // the window: win[k] = y_{i + t0 + k} for the chunk's first left sample i = c0
#pragma unroll
        for (int k = 0; k < ACF_TL; ++k) {
            const int64_t r = c0 + t0 + k;
            const double v = base[nd * (r < last ? r : last)];
            win[k] = (r <= last) ? v - mj : 0.0;
        }
        for (int64_t ib = c0; ib < c1; ib += ACF_TL) {
            // ACF_TL left samples per trip; at step u the window slot (u + k) % ACF_TL holds y_{i + t0 + k}, and after it slot u takes
            // the sample that enters (y_{i + t0 + ACF_TL}): the rotation is in the (compile-time) register names, no moves
#pragma unroll
            for (int ub = 0; ub < ACF_TL; ub += ACF_U) {
                double lf[ACF_U], rt[ACF_U];
#pragma unroll
                for (int u = 0; u < ACF_U; ++u) {
                    const int64_t i = ib + ub + u, r = i + t0 + ACF_TL;
                    const double a = base[nd * (i < last ? i : last)];
                    const double b = base[nd * (r < last ? r : last)];
                    lf[u] = (i < c1) ? a - mj : 0.0;
                    rt[u] = (r <= last) ? b - mj : 0.0;
                }
#pragma unroll
                for (int u = 0; u < ACF_U; ++u) {
#pragma unroll
                    for (int k = 0; k < ACF_TL; ++k) acc[k] = fma(lf[u], win[(ub + u + k) % ACF_TL], acc[k]);
                    win[(ub + u) % ACF_TL] = rt[u];
                }
            }
        }
    }
    double* out = part + lane + nd * ((int64_t)ACF_TL * (blockIdx.y + (int64_t)2 * nchunk * blockIdx.z));
#pragma unroll
    for (int k = 0; k < ACF_TL; ++k) out[nd * k] = acc[k];
}

// grid: x = parameter, y = lag - lag0 (lag0 .. lag0 + gridDim.y - 1, all within the tiles `part` holds); out[p + d (y + out_off)]
__global__ void __launch_bounds__(256) acf_reduce_kernel(const double* part, int64_t N, int d, int nchunk, double* out, int64_t out_off)
{
    __shared__ double ra[256];
    const int p = blockIdx.x;
    const int64_t nd = N * d;
    const int64_t z = blockIdx.y / ACF_TL, k = blockIdx.y % ACF_TL;
    double a = 0.0;
    int64_t h = 0, c = threadIdx.x;              // (h, c) = (j / N, j % N) kept by carrying, as in rhat_reduce_kernel
    while (c >= N) { c -= N; ++h; }
    for (int64_t j = threadIdx.x; j < 2 * N; j += 256) {
        const double* src = part + c + N * p + nd * (k + ACF_TL * (h * nchunk + 2 * nchunk * z));
        double v = 0.0;
        for (int ck = 0; ck < nchunk; ++ck) v += src[nd * ACF_TL * ck];
        a += v;
        c += 256;
        while (c >= N) { c -= N; ++h; }
    }
    ra[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) ra[threadIdx.x] += ra[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[p + (int64_t)d * (blockIdx.y + out_off)] = ra[0];
}

}  // namespace demcz
