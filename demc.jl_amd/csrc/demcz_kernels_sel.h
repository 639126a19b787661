// demcz_kernels_sel.h -- K9: selection over the resident history (gfx950): the counting pass of the quantiles' radix select and
// the arg-max of log_obj (DESIGN.md sections 3 and 4.8).  Integer work only: the counts are exact and do not depend on the
// order in which they are added, so every result is bit-reproducible, also when partial counts are added over shards.
//
//   select_counts_kernel<NP>: one pass over the window.  For parameter p and each of its NP key prefixes u:
//       counts[p][u][b] += #{draws x of p : key(x) >> (shift + 8) == prefix[p][u]  and  (key(x) >> shift) & 255 == b}
//       (at shift 56 there is nothing above the byte: every draw matches, NP = 1), and nan_count[p] += #{x != x}.
//       key(x) is the order-preserving key of demcz_select_host.h.  The prefixes of one parameter are distinct; ~0 pads the list
//       and matches nothing (a key shifted right by at least 8 has zero top bits).
//   best_partial_kernel / best_final_kernel: arg-max of (value, linear index) over a contiguous range of log_obj: the larger
//       value wins, on == the smaller index, a NaN is never a candidate.  One partial per workgroup, one workgroup finishes.
//
// No waits between waves, no spin loops, no floating-point atomics.
#pragma once

#include "demcz_device.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int SEL_BS = 256;     // four waves: they share the 64 chains and the histogram, and take the generations in turn
constexpr int SEL_U = 4;        // generations a wave loads before it counts them: four 512-byte runs in flight per wave

__device__ __forceinline__ uint64_t sel_key(uint64_t b) { return (b >> 63) ? ~b : (b | (1ull << 63)); }

// grid: x = parameter * cb + chain block of 64 (a workgroup stays inside one parameter: its prefixes are wave-uniform),
//       y = time chunk of `per` generations.   prefix: [d][NP];  counts: [d][NP][256];  nan_count: [d].
//
// Bounds: a load is of chain c < N, parameter p < d and slot s0 + g with 0 <= g < w, under the lane's own predicate: inside the
// window check_hist_range admitted.  A histogram index is u * 256 + (byte & 255) with u < NP.
template <int NP>
__global__ void __launch_bounds__(SEL_BS) select_counts_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t w,
                                                               int64_t cb, int64_t per, int shift, const uint64_t* __restrict__ prefix,
                                                               unsigned long long* counts, unsigned long long* nan_count)
{
    __shared__ unsigned int hist[NP * 256];
    __shared__ unsigned int nans;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p = blockIdx.x / cb, c = (blockIdx.x % cb) * 64 + lane;
    const bool valid = c < N;
    const int64_t nd = N * d;
    const int64_t g_lo = (int64_t)blockIdx.y * per, g_hi = (g_lo + per < w) ? g_lo + per : w;

    uint64_t pre[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) pre[u] = prefix[p * NP + u];
    for (int i = tid; i < NP * 256; i += SEL_BS) hist[i] = 0u;
    if (tid == 0) nans = 0u;
    __syncthreads();

    const double* base = chain + (valid ? c : 0) + N * p + nd * s0;
    // a run of wave-uniform hits (every counting lane of the wave in one bin, the usual case in the first passes of a posterior
    // away from zero) is kept in scalars and added once when the bin changes
    int pend_code = -1;
    unsigned int pend_cnt = 0u, nan_cnt = 0u;
    for (int64_t gb = g_lo + (int64_t)wv * SEL_U; gb < g_hi; gb += (int64_t)(SEL_BS / 64) * SEL_U) {
        uint64_t bits[SEL_U];
        bool ok[SEL_U];
#pragma unroll
        for (int k = 0; k < SEL_U; ++k) {
            ok[k] = valid && gb + k < g_hi;
            bits[k] = ok[k] ? (uint64_t)__double_as_longlong(base[nd * (gb + k)]) : 0ull;
        }
#pragma unroll
        for (int k = 0; k < SEL_U; ++k) {
            const bool isnan = ok[k] && (bits[k] & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
            nan_cnt += (unsigned int)__popcll(__ballot(isnan));
            const uint64_t key = sel_key(bits[k]);
            const uint64_t hi = (shift == 56) ? 0ull : key >> (shift + 8);
            int idx = -1;
#pragma unroll
            for (int u = NP - 1; u >= 0; --u) idx = (hi == pre[u]) ? u : idx;
            const int code = (ok[k] && idx >= 0) ? idx * 256 + (int)((key >> shift) & 255ull) : -1;
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
    if (nan_cnt && lane == 0) atomicAdd(&nans, nan_cnt);
    __syncthreads();
    unsigned long long* out = counts + p * (NP * 256);
    for (int i = tid; i < NP * 256; i += SEL_BS) {
        const unsigned int v = hist[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
    if (tid == 0 && nans) atomicAdd(&nan_count[p], (unsigned long long)nans);
}

// a beats b
__device__ __forceinline__ bool best_beats(double av, long long ai, double bv, long long bi)
{
    return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

__device__ __forceinline__ void best_block_reduce(double& v, long long& i, double* rv, long long* ri)
{
    rv[threadIdx.x] = v;
    ri[threadIdx.x] = i;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && best_beats(rv[threadIdx.x + s], ri[threadIdx.x + s], rv[threadIdx.x], ri[threadIdx.x])) {
            rv[threadIdx.x] = rv[threadIdx.x + s];
            ri[threadIdx.x] = ri[threadIdx.x + s];
        }
        __syncthreads();
    }
    v = rv[0];
    i = ri[0];
}

// lo: the window's first entry; total = N * w entries, read at indices below total only.  pv / pi: gridDim.x partials.
__global__ void __launch_bounds__(256) best_partial_kernel(const double* __restrict__ lo, int64_t total, double* pv, long long* pi)
{
    __shared__ double rv[256];
    __shared__ long long ri[256];
    double bv = __longlong_as_double(0x7ff8000000000000ll);
    long long bi = -1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const double v = lo[i];
        if (v == v && best_beats(v, i, bv, bi)) { bv = v; bi = i; }
    }
    best_block_reduce(bv, bi, rv, ri);
    if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// one workgroup: out_v[0], out_i[0] = the best of nb partials (NaN, -1 when there was no candidate)
__global__ void __launch_bounds__(256) best_final_kernel(const double* pv, const long long* pi, int nb, double* out_v, long long* out_i)
{
    __shared__ double rv[256];
    __shared__ long long ri[256];
    double bv = __longlong_as_double(0x7ff8000000000000ll);
    long long bi = -1;
    for (int k = threadIdx.x; k < nb; k += 256)
        if (best_beats(pv[k], pi[k], bv, bi)) { bv = pv[k]; bi = pi[k]; }
    best_block_reduce(bv, bi, rv, ri);
    if (threadIdx.x == 0) { out_v[0] = bv; out_i[0] = bi; }
}

}  // namespace demcz
