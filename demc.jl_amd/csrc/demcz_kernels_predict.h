// demcz_kernels_predict.h -- posterior predictive programs (demcz_predict and demcz_ppc, include/demcz.h; DESIGN.md sections 3
// and 4.19; gfx950): a user-written function of every draw of a history window AND of the draw's own random stream.
//
// Compiled at run time only, in a unit of its own (demcz_program.hip, compose: UNIT_PREDICT) that defines DEMCZ_PREDICT_UNIT,
// DEMCZ_D and DEMCZ_M and holds, in front of this header, demcz_device.h, demcz_predict_rng.h and the user's
//     __device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out);
//
//   predict_kernel   derive_kernel's stream (demcz_kernels_derive.h): one lane per draw i = c + N t, 256 lanes, strided over at most
//                    DERIVE_MAX_WG workgroups, 64-bit indices, (i, c, t) advanced without a division in the loop; out is an
//                    N x DEMCZ_M x w derived history.
//   ppc_kernel       the same calls, no history: out[k] is compared with observed[k] and three counts per k -- greater, equal,
//                    out[k] is NaN -- are added into counts[3 DEMCZ_M] (counts[3 k], [3 k + 1], [3 k + 2]).
// The lane of draw (c, t) seeds its demcz_rng from (seed, g0 + t, chain_id0 + c): what a draw is given does not depend on the
// window, the launch, the shard or the history's origin.  x and o are indexed by unrolled compile-time loops only and live in
// registers.
//
// Bounds.  Every load and store of the stream is under the lane's own predicate i < total, i = c + N t, c < N, t < w:
// chain[c + N (p + DEMCZ_D (s0 + t))] with p < DEMCZ_D and s0 + t < Gcap (the host checks the window); logobj[c + N (s0 + t)];
// out[c + N (k + DEMCZ_M t)] with k < DEMCZ_M, an N x DEMCZ_M x w array; observed[k] and counts[3 k + j] with k < DEMCZ_M, j < 3, at
// compile-time k (the host sizes both); the LDS words part[wave][j] with wave < 4, j < 3 DEMCZ_M.
#pragma once

#include <stdint.h>

#include "demcz_kernels_derive.h"

#ifdef DEMCZ_PREDICT_UNIT
namespace demcz {

// One draw: its parameters and log_obj loaded, o preset to NaN, the rng seeded, the user's function called
__device__ __forceinline__ void predict_draw(const double* __restrict__ chain, const double* __restrict__ logobj, int64_t N, int64_t slot,
                                             int64_t c, const double* __restrict__ data, int64_t ndata, uint64_t seed, uint32_t g,
                                             uint32_t cglobal, double (&o)[DEMCZ_M])
{
    const double* src = chain + c + N * DEMCZ_D * slot;
    double x[DEMCZ_D];
#pragma unroll
    for (int p = 0; p < DEMCZ_D; ++p) x[p] = src[N * p];
    const double logp = logobj ? logobj[c + N * slot] : __builtin_nan("");
#pragma unroll
    for (int k = 0; k < DEMCZ_M; ++k) o[k] = __builtin_nan("");
    demcz_rng rng;
    demcz_rng_seed(&rng, seed, g, cglobal);
    demcz_predict(x, logp, data, ndata, &rng, o);
}

__global__ __launch_bounds__(DERIVE_THREADS) void predict_kernel(const double* __restrict__ chain, const double* __restrict__ logobj,
                                                                int64_t N, int64_t s0, int64_t total,
                                                                const double* __restrict__ data, int64_t ndata, uint64_t seed,
                                                                int64_t g0, int64_t chain_id0, double* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t i = (int64_t)blockIdx.x * DERIVE_THREADS + threadIdx.x;
    int64_t t = i / N, c = i - t * N;
    for (; i < total; i += stride) {
        double o[DEMCZ_M];
        predict_draw(chain, logobj, N, s0 + t, c, data, ndata, seed, (uint32_t)(g0 + t), (uint32_t)(chain_id0 + c), o);
        double* dst = out + c + N * DEMCZ_M * t;
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) dst[N * k] = o[k];
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
}

// The stride loop is the wave's, not the lane's: `base`, the draw of the wave's lane 0, is the same value in all 64 lanes, so every
// lane makes every pass and the ballots below are taken by whole waves; a lane past the end of the window (live == false) calls
// nothing, loads nothing and is in none of the three masks.  The counts of a wave are wave-uniform 32-bit values (a wave adds at most
// 64 a pass, and a window that overflowed them -- 2^45 draws -- fits no device); integers throughout, so the totals do not depend
// on how the window is cut, the chains are sharded or the adds are ordered.
__global__ __launch_bounds__(DERIVE_THREADS) void ppc_kernel(const double* __restrict__ chain, const double* __restrict__ logobj,
                                                            int64_t N, int64_t s0, int64_t total,
                                                            const double* __restrict__ data, int64_t ndata, uint64_t seed,
                                                            int64_t g0, int64_t chain_id0, const double* __restrict__ observed,
                                                            unsigned long long* __restrict__ counts)
{
    constexpr int WAVES = DERIVE_THREADS / 64;
    __shared__ unsigned int part[WAVES][3 * DEMCZ_M];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t base = (int64_t)blockIdx.x * DERIVE_THREADS + wave * 64;
    int64_t t = (base + lane) / N, c = (base + lane) - t * N;
    unsigned int gt[DEMCZ_M], eq[DEMCZ_M], nn[DEMCZ_M];
#pragma unroll
    for (int k = 0; k < DEMCZ_M; ++k) gt[k] = eq[k] = nn[k] = 0u;
    for (; base < total; base += stride) {
        const bool live = base + lane < total;
        double o[DEMCZ_M];
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) o[k] = 0.0;
        if (live) predict_draw(chain, logobj, N, s0 + t, c, data, ndata, seed, (uint32_t)(g0 + t), (uint32_t)(chain_id0 + c), o);
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) {
            const double y = observed[k];
            gt[k] += (unsigned int)__popcll(__ballot(live && o[k] > y));
            eq[k] += (unsigned int)__popcll(__ballot(live && o[k] == y));
            nn[k] += (unsigned int)__popcll(__ballot(live && o[k] != o[k]));
        }
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) {
            part[wave][3 * k] = gt[k];
            part[wave][3 * k + 1] = eq[k];
            part[wave][3 * k + 2] = nn[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * DEMCZ_M) {
        unsigned long long s = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) s += part[v][threadIdx.x];
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

}  // namespace demcz
#endif
