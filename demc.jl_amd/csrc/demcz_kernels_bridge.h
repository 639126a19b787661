// demcz_kernels_bridge.h -- K12: the marginal likelihood by bridge sampling (demcz_bridge, include/demcz.h; DESIGN.md sections 3
// and 4.17; gfx950).  The proposal is g = N(m, L L^T); mL holds what every lane reads of it, the same words in every lane:
//     mL[p]                                   m_p                         p < D
//     mL[D + p (p + 1) / 2 + q]               L_pq, row-major lower       q <= p < D
// BRIDGE_ML_WORDS(D) = D + D (D + 1) / 2 doubles in all, read through a const __restrict__ kernel argument at compile-time
// offsets: wave-uniform addresses, which the compiler turns into scalar loads.
//
//   bridge_posterior_kernel<D>     a1 = log_obj - log g(x) of every draw of a history window (the solve L z = x - m)
//   bridge_proposal_kernel<T, D>   fresh draws x = m + L z from Philox and Box-Muller, a2 = logobj(x) - log g(x); built-in targets
//   bridge_proposal_program_kernel the same for a program target, compiled at run time in a unit of its own (demcz_program.hip,
//                                  UNIT_BRIDGE: DEMCZ_BRIDGE_UNIT, DEMCZ_D, the user's demcz_logobj, demcz_device.h, this header)
//   bridge_rho0_kernel             rho_0 = max a1: a launch over the tiles of a1, then one workgroup over the tiles' maxima
//   bridge_sum_kernel              grid (tiles of 1024, 2): the tile partials of f1 (y = 0) and f2 (y = 1) at the rho in device memory
//   bridge_finish_kernel           one workgroup: each sum's tiles added in index order by one lane, rho', the stopping test
//
// The first three are derive_kernel's stream (demcz_kernels_derive.h): one lane per draw, 256 lanes, strided over at most 2048
// workgroups, 64-bit indices, (i, c, t) advanced without a division in the loop.  x and z are indexed by unrolled compile-time
// loops only and live in registers.
//
// Bounds.  Every load and store of the three streaming kernels is under the lane's own predicate i < total, i = c + N t, c < N,
// t < w:  chain[c + N (p + D (s0 + t))] with p < D and s0 + t < Gcap (the host checks the window);  logobj[c + N (s0 + t)];
// a1[c + N t] = a1[i];  a2[i];  draws[c + N (p + D t)] with p < D, an N x D x w array;  mL[k] with k < BRIDGE_ML_WORDS(D) at
// compile-time k.  bridge_rho0_kernel loads a1[i] under i < n1 and stores part[tile], tile < tiles(n1) = its grid (stage 0), or loads
// part[t], t < tiles(n1), and stores the state's rho (stage 1).  bridge_sum_kernel loads a[i] under
// i < n (n = n2 for y = 0, n1 for y = 1), stores f2[i] under the same predicate where f2 is not null, and part[(y ntiles + tile)
// BRIDGE_NPART + q] with tile < ntiles = gridDim.x (the host sizes part for max(tiles of n1, tiles of n2) per y) and
// q < BRIDGE_NPART.  bridge_finish_kernel loads the same part words for tile < tiles(n_y) and touches the one BridgeState.
#pragma once

#include <stdint.h>

#include "demcz_device.h"
#include "demcz_kernels_derive.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int BRIDGE_MAX_D = 32;
constexpr int BRIDGE_BS = 256;                          // four waves
constexpr int BRIDGE_KPT = 4;                           // elements per lane and tile
constexpr int BRIDGE_TILE = BRIDGE_BS * BRIDGE_KPT;     // 1024
constexpr int BRIDGE_NPART = 4;                         // per tile: sum (f - shift), sum (f - shift)^2, refused entries, NaN entries
constexpr int BRIDGE_ML_WORDS_MAX = BRIDGE_MAX_D + BRIDGE_MAX_D * (BRIDGE_MAX_D + 1) / 2;

__host__ __device__ constexpr int bridge_ml_words(int d) { return d + d * (d + 1) / 2; }

// log g of the standardised z: s = sum z_p^2 by fma in index order from 0, -0.5 s - c_g
template <int D>
__device__ __forceinline__ double bridge_logg(const double (&z)[D], double cg)
{
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) s = fma(z[p], z[p], s);
    return -0.5 * s - cg;
}

// Draw j = c + N t of the proposal: z_2k, z_2k+1 are the Box-Muller pair of Philox block t B + k of stream (seed, c), B = ceil(D / 2)
// (for odd D the last value is unused); x_p = m_p + sum_{q <= p} L_pq z_q by fma in index order.
template <int D>
__device__ __forceinline__ void bridge_draw(uint64_t seed, int64_t c, int64_t t, const double* __restrict__ mL, double (&z)[D], double (&x)[D])
{
    constexpr int B = (D + 1) / 2;
    rng_state st;
    rng_seek(st, seed, (uint64_t)c, (uint64_t)t * B);
#pragma unroll
    for (int k = 0; k < B; ++k) {
        uint64_t r1, r2;
        rng_next(st, r1, r2);
        double z0, z1;
        normal_pair(r1, r2, z0, z1);
        z[2 * k] = z0;
        if (2 * k + 1 < D) z[(2 * k + 1 < D) ? 2 * k + 1 : 0] = z1;
    }
#pragma unroll
    for (int p = 0; p < D; ++p) {
        double acc = mL[p];
#pragma unroll
        for (int q = 0; q <= p; ++q) acc = fma(mL[D + p * (p + 1) / 2 + q], z[q], acc);
        x[p] = acc;
    }
}

// the stream over the N x w draws of the proposal; LOGP: x[D] -> the target's log-density
template <int D, class LOGP>
__device__ __forceinline__ void bridge_proposal_stream(int64_t N, int64_t total, uint64_t seed, const double* __restrict__ mL, double cg,
                                                       double* __restrict__ a2, double* __restrict__ draws, LOGP logp)
{
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t i = (int64_t)blockIdx.x * DERIVE_THREADS + threadIdx.x;
    int64_t t = i / N, c = i - t * N;
    for (; i < total; i += stride) {
        double z[D], x[D];
        bridge_draw<D>(seed, c, t, mL, z, x);
        const double logg = bridge_logg<D>(z, cg);
        a2[i] = logp(x) - logg;
        if (draws) {
            double* dst = draws + c + N * D * t;
#pragma unroll
            for (int p = 0; p < D; ++p) dst[N * p] = x[p];
        }
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
}

}  // namespace demcz

#ifdef DEMCZ_BRIDGE_UNIT
// ---- the program unit: the user's demcz_logobj stands in front of this header ---------------------------------------------------
namespace demcz {

__global__ __launch_bounds__(DERIVE_THREADS) void bridge_proposal_program_kernel(int64_t N, int64_t total, uint64_t seed,
                                                                                const double* __restrict__ mL, double cg,
                                                                                const double* __restrict__ data, int64_t ndata,
                                                                                double* __restrict__ a2, double* __restrict__ draws)
{
    bridge_proposal_stream<DEMCZ_D>(N, total, seed, mL, cg, a2, draws,
                                    [&](const double (&x)[DEMCZ_D]) { return demcz_logobj(x, data, ndata); });
}

}  // namespace demcz
#else
// ---- the library's side: behind demcz_kernels.h; the kernels themselves only in demcz_bridge_inst.hip (DEMCZ_BRIDGE_INST) -----------
namespace demcz {

// the iteration's state, one per call, in device memory
struct BridgeState {
    double rho;              // the current rho (rho_0 = max a1 before the first update)
    double mean[2];          // mean f1, mean f2 of the latest sums
    double var[2];           // the final launch: their variances, divisor n
    double n_nan;            // NaN entries of a2 (they count as -inf)
    long long iterations;    // updates made
    int done;                // set: launches queued behind leave everything alone
    int converged;
};

// the kernels by dimension and target (demcz_bridge_inst.hip; nullptr where there is none): demcz_capi.hip launches them through
// these and does not instantiate them
const void* bridge_posterior_fn(int d);
const void* bridge_proposal_fn(int target_kind, int d);
const void* bridge_rho0_fn();
const void* bridge_sum_fn();
const void* bridge_finish_fn();

}  // namespace demcz

#ifdef DEMCZ_BRIDGE_INST
namespace demcz {

template <int D>
__global__ __launch_bounds__(DERIVE_THREADS) void bridge_posterior_kernel(const double* __restrict__ chain, const double* __restrict__ logobj,
                                                                         int64_t N, int64_t s0, int64_t total,
                                                                         const double* __restrict__ mL, double cg, double* __restrict__ a1)
{
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t i = (int64_t)blockIdx.x * DERIVE_THREADS + threadIdx.x;
    int64_t t = i / N, c = i - t * N;
    for (; i < total; i += stride) {
        const int64_t slot = s0 + t;
        const double* src = chain + c + N * D * slot;
        double z[D];
#pragma unroll
        for (int p = 0; p < D; ++p) {
            double acc = src[N * p] - mL[p];
#pragma unroll
            for (int k = 0; k < p; ++k) acc = fma(-mL[D + p * (p + 1) / 2 + k], z[k], acc);
            z[p] = acc / mL[D + p * (p + 1) / 2 + p];
        }
        a1[i] = logobj[c + N * slot] - bridge_logg<D>(z, cg);
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
}

template <int TARGET, int D>
__global__ __launch_bounds__(DERIVE_THREADS) void bridge_proposal_kernel(TargetParams tp, int64_t N, int64_t total, uint64_t seed,
                                                                        const double* __restrict__ mL, double cg,
                                                                        double* __restrict__ a2, double* __restrict__ draws)
{
    bridge_proposal_stream<D>(N, total, seed, mL, cg, a2, draws,
                              [&](const double (&x)[D]) { return target_logp<TARGET, D>(tp, D, [&](int j) { return x[j]; }); });
}

// every lane gets the same sum: v[l] + v[l ^ 32], then ^ 16, ... ^ 1; then the four waves in order.  red: 4 doubles of LDS
__device__ __forceinline__ double bridge_block_sum(double v, double* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                                     // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// rho_0 = max a1 in two launches; a NaN among them is ignored here (fmax), the sums refuse it.  stage 0, grid = the tiles of n1:
// a tile's maximum -> part[tile].  stage 1, one workgroup: the maximum of the tiles -> the state's rho.  (A maximum does not
// depend on the order it is taken in.)
__global__ __launch_bounds__(BRIDGE_BS) void bridge_rho0_kernel(const double* __restrict__ a1, int64_t n1, int64_t tiles, int stage,
                                                               double* __restrict__ part, BridgeState* __restrict__ st)
{
    __shared__ double red[BRIDGE_BS / 64];
    double m = -__builtin_inf();
    if (stage == 0) {
#pragma unroll
        for (int kk = 0; kk < BRIDGE_KPT; ++kk) {
            const int64_t i = (int64_t)blockIdx.x * BRIDGE_TILE + kk * BRIDGE_BS + threadIdx.x;
            if (i < n1) m = fmax(m, a1[i]);
        }
    } else {
        for (int64_t t = threadIdx.x; t < tiles; t += BRIDGE_BS) m = fmax(m, part[t]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (stage == 0) part[blockIdx.x] = m; else st->rho = m;
}

// grid (ntiles, 2).  y = 0: f1 = 1 / (s1 + s2 exp(rho - a2)) over the n2 proposal draws, a NaN a2 counted and taken as -inf (f1 = 0),
// a +inf a2 refused.  y = 1: f2 = 1 / (s1 exp(a1 - rho) + s2) over the n1 posterior draws, a non-finite a1 refused.  An exp that
// overflows gives the term's limit 0.  final = 0: an update's sums, shift 0, skipped behind a set done flag.  final = 1: the
// moments' sums at the final rho, shifted by the latest means (the variance then loses nothing to cancellation), and f2 stored.
__global__ __launch_bounds__(BRIDGE_BS) void bridge_sum_kernel(const double* __restrict__ a2, int64_t n2, const double* __restrict__ a1,
                                                              int64_t n1, double s1, double s2, int final,
                                                              const BridgeState* __restrict__ st, double* __restrict__ part,
                                                              double* __restrict__ f2)
{
    __shared__ double red[BRIDGE_BS / 64];
    if (!final && st->done) return;                                      // uniform over the grid
    const int y = blockIdx.y;
    const int64_t n = y ? n1 : n2;
    if ((int64_t)blockIdx.x * BRIDGE_TILE >= n) return;                  // uniform over the workgroup: a tile of the longer side only
    const double* __restrict__ a = y ? a1 : a2;
    const double rho = st->rho, shift = final ? st->mean[y] : 0.0;
    double s[BRIDGE_NPART] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < BRIDGE_KPT; ++kk) {
        const int64_t i = (int64_t)blockIdx.x * BRIDGE_TILE + kk * BRIDGE_BS + threadIdx.x;
        if (i < n) {
            const double v = a[i];
            double f;
            if (y == 0) {
                const bool isnan = v != v;
                f = isnan ? 0.0 : 1.0 / (s1 + s2 * exp(rho - v));
                s[2] += (v == __builtin_inf()) ? 1.0 : 0.0;
                s[3] += isnan ? 1.0 : 0.0;
            } else {
                f = 1.0 / (s1 * exp(v - rho) + s2);
                s[2] += (v - v == 0.0) ? 0.0 : 1.0;
                if (final && f2) f2[i] = f;
            }
            const double dv = f - shift;
            s[0] += dv;
            s[1] += dv * dv;
        }
    }
    double* out = part + ((int64_t)y * gridDim.x + blockIdx.x) * BRIDGE_NPART;
#pragma unroll
    for (int q = 0; q < BRIDGE_NPART; ++q) {
        const double v = bridge_block_sum(s[q], red);
        if (threadIdx.x == 0) out[q] = v;
    }
}

// One workgroup.  Each of the eight sums (two sides, BRIDGE_NPART partials) is added by one lane of its own, the tiles in index
// order from 0 (eight loads in flight, added in order); lane 0 then does the rest.  final = 0: rho' = (rho + log mean f1) -
// log mean f2, the update count, the stopping test |rho' - rho| <= tol or max_iter updates; a refused entry or a mean that is 0
// ends it with rho = NaN.  final = 1: the means and variances (divisor n) at the final rho and the NaN count.
__global__ __launch_bounds__(64) void bridge_finish_kernel(const double* __restrict__ part, int64_t ntiles, int64_t n2, int64_t n1,
                                                          double tol, long long max_iter, int final, BridgeState* __restrict__ st)
{
    __shared__ double tot[2 * BRIDGE_NPART];
    if (!final && st->done) return;                                      // uniform over the workgroup
    const int l = threadIdx.x;
    if (l < 2 * BRIDGE_NPART) {
        const int y = l / BRIDGE_NPART, q = l % BRIDGE_NPART;
        const int64_t n = y ? n1 : n2, tiles = (n + BRIDGE_TILE - 1) / BRIDGE_TILE;
        const double* p = part + (int64_t)y * ntiles * BRIDGE_NPART + q;
        double s = 0.0;
        int64_t t = 0;
        for (; t + 8 <= tiles; t += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(t + u) * BRIDGE_NPART];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; t < tiles; ++t) s += p[t * BRIDGE_NPART];
        tot[l] = s;
    }
    __syncthreads();
    if (l != 0) return;
    double mean[2], var[2], refused = 0.0, nnan = 0.0;
    for (int y = 0; y < 2; ++y) {
        const int64_t n = y ? n1 : n2;
        const double* s = tot + y * BRIDGE_NPART;
        const double dn = (double)n, ms = s[0] / dn;
        mean[y] = final ? st->mean[y] + ms : ms;
        var[y] = s[1] / dn - ms * ms;
        refused += s[2];
        if (y == 0) nnan = s[3];
    }
    st->n_nan = nnan;
    if (final) {
        st->mean[0] = mean[0]; st->mean[1] = mean[1];
        st->var[0] = var[0] > 0.0 ? var[0] : 0.0;
        st->var[1] = var[1] > 0.0 ? var[1] : 0.0;
        return;
    }
    st->mean[0] = mean[0]; st->mean[1] = mean[1];
    if (refused != 0.0 || !(mean[0] > 0.0) || !(mean[1] > 0.0)) {
        st->rho = __builtin_nan("");
        st->done = 1;
        st->converged = 0;
        return;
    }
    const double rho = st->rho, next = (rho + log(mean[0])) - log(mean[1]);
    const long long it = st->iterations + 1;
    st->iterations = it;
    st->rho = next;
    if (fabs(next - rho) <= tol) { st->converged = 1; st->done = 1; }
    else if (it >= max_iter) st->done = 1;
}

}  // namespace demcz
#endif  // DEMCZ_BRIDGE_INST
#endif
