// demcz_kernels_rank.h -- K10: exact average ranks of every draw of a history window among all S = N w draws of its parameter,
// their normal scores, and the indicator columns of the tail ESS (gfx950; DESIGN.md sections 3 and 4.14).
//
// The value ranked is v = x (bulk) or fabs(x - center[p]) (folded), then v + 0.0 so that -0.0 ranks as +0.0; its key is the
// order-preserving key of the quantiles (sel_key, demcz_kernels_sel.h).  Per parameter the S keys are sorted, keys only, by an
// LSD radix sort with 8-bit digits between two buffers; a draw's rank is then less + (equal + 1) / 2 from the lower and the upper
// bound of its key in the sorted array.  All parameters go through the same launches (blockIdx.y = parameter).
//
//   rank_keys_kernel        reads the window once: writes the keys in draw order (i = c + N t) and adds all eight 256-bin digit
//                           histograms and the NaN count of each parameter (8 KB of LDS counters per workgroup)
//   -- the host reads the histograms: a digit whose histogram has one bin holding all S keys is skipped for that parameter --
//   rank_tile_count_kernel  per tile of RANK_TILE keys: the 256 counts of the pass's digit              -> tcount[p][digit][tile]
//   rank_tile_scan_kernel   per (parameter, digit): exclusive scan of the digit's counts over the tiles, in place, started at the
//                           number of keys with a smaller digit (the host has it from the histograms): together the exclusive
//                           scan in (digit, tile) order
//   rank_scatter_kernel     per tile: every wave owns RANK_KPT runs of 64 consecutive keys; eight ballots give a lane the mask
//                           of the lanes with its digit, popc(mask & lanes below) its place among them: the tile is placed stably
//   rank_score_kernel       one lane per draw: lower and upper bound of its key, the rank, demcz_rank_host.h's rank -> z (or the
//                           rank itself), written straight into the N x d x w derived history
//   indicator_le_kernel     out[c, p + d u, g] = (x <= thr[p + d u]) ? 1 : 0, NaN stays NaN
//
// Launch boundaries separate histogram, count, scan and scatter: no waits between workgroups, no spin loops.  Integer work up to
// the rank, so the ranks are exact and do not depend on the order of any addition; no floating-point atomics.
//
// Bounds: a history load is of chain c < N, parameter p < d (p = blockIdx.y < gridDim.y = d) and slot s0 + t with t < w, under
// the lane's own predicate i = c + N t < S; a key load or store is at p S + i with i < S under the same predicate; a scatter
// store is at p S + pos, pos being the lane's place in the exclusive scan of the very counts the same keys produced, and is
// predicated on pos < S besides; the searches of rank_score_kernel read sorted[mid] with lo <= mid < hi <= S and sorted[hi] with
// hi < S.  Histogram and tile-count indices are digit < 256 within [p][8][256] and [p][256][tile < ntiles].
#pragma once

#include "demcz_device.h"
#include "demcz_kernels_sel.h"
#include "demcz_rank_host.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int RANK_BS = 256;                        // four waves
constexpr int RANK_KPT = 4;                         // keys per lane and tile
constexpr int RANK_TILE = RANK_BS * RANK_KPT;       // 1024 keys: a wave owns 256 consecutive ones
constexpr int RANK_DIGITS = 8;

// the value ranked: x, or fabs(x - center) (one rounded subtraction); + 0.0 turns -0.0 into +0.0
__device__ __forceinline__ double rank_value_of(double x, bool folded, double center)
{
    double v = x;
    if (folded) {
        const double diff = x - center;
        v = fabs(diff);
    }
    return v + 0.0;
}

__device__ __forceinline__ uint64_t rank_key_of(double v) { return sel_key((uint64_t)__double_as_longlong(v)); }

// hist[bin] += the number of counting lanes of the wave whose bin it is: one add when the whole wave agrees (the usual case in
// the top digits of a posterior away from zero), one per lane otherwise
__device__ __forceinline__ void rank_wave_count(unsigned int* hist, int bin, bool ok, int lane)
{
    const unsigned long long m = __ballot(ok);
    if (!m) return;                                                      // wave-uniform
    const int lead = __ffsll(m) - 1;
    const int first = __builtin_amdgcn_readlane(bin, lead);
    const unsigned long long same = __ballot(ok && bin == first);
    if (same == m) {
        if (lane == lead) atomicAdd(&hist[first], (unsigned int)__popcll(m));
    } else if (ok) {
        atomicAdd(&hist[bin], 1u);
    }
}

// grid: x = tile of RANK_TILE draws, y = parameter.  keys: [d][S];  hist: [d][8][256];  nan_count: [d];  center: d values or null.
__global__ void __launch_bounds__(RANK_BS) rank_keys_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t S,
                                                            const double* __restrict__ center, uint64_t* __restrict__ keys,
                                                            unsigned long long* hist, unsigned long long* nan_count)
{
    __shared__ unsigned int lh[RANK_DIGITS * 256];
    __shared__ unsigned int nans;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p = blockIdx.y;
    const bool folded = center != nullptr;
    const double ctr = folded ? center[p] : 0.0;
    for (int i = tid; i < RANK_DIGITS * 256; i += RANK_BS) lh[i] = 0u;
    if (tid == 0) nans = 0u;
    __syncthreads();
    unsigned int nan_cnt = 0u;
#pragma unroll
    for (int k = 0; k < RANK_KPT; ++k) {
        const int64_t i = (int64_t)blockIdx.x * RANK_TILE + k * RANK_BS + tid;
        const bool ok = i < S;
        const int64_t t = ok ? i / N : 0, c = ok ? i - t * N : 0;
        const double x = ok ? chain[c + N * p + N * d * (s0 + t)] : 0.0;
        const double v = rank_value_of(x, folded, ctr);
        const uint64_t key = rank_key_of(v);
        if (ok) keys[p * S + i] = key;
        nan_cnt += (unsigned int)__popcll(__ballot(ok && v != v));
#pragma unroll
        for (int b = 0; b < RANK_DIGITS; ++b) rank_wave_count(lh + b * 256, (int)((key >> (8 * b)) & 255ull), ok, lane);
    }
    if (nan_cnt && lane == 0) atomicAdd(&nans, nan_cnt);
    __syncthreads();
    unsigned long long* out = hist + p * (RANK_DIGITS * 256);
    for (int i = tid; i < RANK_DIGITS * 256; i += RANK_BS) {
        const unsigned int v = lh[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
    if (tid == 0 && nans) atomicAdd(&nan_count[p], (unsigned long long)nans);
}

// info[p]: -1 the parameter skips this pass, 0 its keys are in buf0, 1 in buf1.
// grid: x = tile, y = parameter.  tcount: [d][256][ntiles].
__global__ void __launch_bounds__(RANK_BS) rank_tile_count_kernel(const uint64_t* __restrict__ buf0, const uint64_t* __restrict__ buf1,
                                                                  int64_t S, int64_t ntiles, int shift, const int* __restrict__ info,
                                                                  unsigned int* __restrict__ tcount)
{
    __shared__ unsigned int lh[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p = blockIdx.y;
    const int which = info[p];
    if (which < 0) return;                                               // uniform over the workgroup
    const uint64_t* src = (which ? buf1 : buf0) + p * S;
    lh[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RANK_KPT; ++k) {
        const int64_t i = (int64_t)blockIdx.x * RANK_TILE + k * RANK_BS + tid;
        const bool ok = i < S;
        const uint64_t key = ok ? src[i] : 0ull;
        rank_wave_count(lh, (int)((key >> shift) & 255ull), ok, lane);
    }
    __syncthreads();
    tcount[(p * 256 + tid) * ntiles + blockIdx.x] = lh[tid];
}

// grid: x = digit, y = parameter; 256 lanes walk the digit's row of ntiles counts in chunks of 256 with a running carry.  In
// place: tcount[p][b][t] becomes dbase[p][b] + the number of keys with digit b in a tile before t -- where tile t's first key of
// digit b goes.  dbase[p][b]: the number of keys of parameter p with a smaller digit, from the first kernel's histogram.
__global__ void __launch_bounds__(256) rank_tile_scan_kernel(int64_t ntiles, const int* __restrict__ info,
                                                             const unsigned int* __restrict__ dbase, unsigned int* tcount)
{
    __shared__ unsigned int tmp[256];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.y, b = blockIdx.x;
    if (info[p] < 0) return;                                             // uniform over the workgroup
    unsigned int* row = tcount + (p * 256 + b) * ntiles;
    unsigned int carry = dbase[p * 256 + b];
    for (int64_t t0 = 0; t0 < ntiles; t0 += 256) {
        const int64_t t = t0 + tid;
        const unsigned int v = (t < ntiles) ? row[t] : 0u;
        tmp[tid] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                              // inclusive scan over the chunk
            const unsigned int add = (tid >= s) ? tmp[tid - s] : 0u;
            __syncthreads();
            tmp[tid] += add;
            __syncthreads();
        }
        if (t < ntiles) row[t] = carry + tmp[tid] - v;
        carry += tmp[255];
        __syncthreads();                                                 // (tmp is rewritten by the next chunk)
    }
}

// the lanes of the wave that count (ok) and hold the same digit as this one; 0 for a lane that does not count
__device__ __forceinline__ unsigned long long rank_peers(int digit, bool ok)
{
    unsigned long long peers = __ballot(ok);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool set = (digit >> bit) & 1;
        const unsigned long long m = __ballot(set);
        peers &= set ? m : ~m;
    }
    return ok ? peers : 0ull;
}

// grid: x = tile, y = parameter.  toff: rank_tile_scan_kernel's output.  Wave v of the tile owns keys [256 v, 256 v + 256) of
// it, in RANK_KPT runs of 64: the order of the keys of one digit is (wave, run, lane) = their order in the source.
__global__ void __launch_bounds__(RANK_BS) rank_scatter_kernel(uint64_t* __restrict__ buf0, uint64_t* __restrict__ buf1, int64_t S,
                                                               int64_t ntiles, int shift, const int* __restrict__ info,
                                                               const unsigned int* __restrict__ toff)
{
    __shared__ unsigned int wcnt[RANK_BS / 64][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p = blockIdx.y;
    const int which = info[p];
    if (which < 0) return;                                               // uniform over the workgroup
    const uint64_t* src = (which ? buf1 : buf0) + p * S;
    uint64_t* dst = (which ? buf0 : buf1) + p * S;
#pragma unroll
    for (int v = 0; v < RANK_BS / 64; ++v) wcnt[v][tid] = 0u;
    __syncthreads();
    uint64_t key[RANK_KPT];
    bool ok[RANK_KPT];
    const int64_t base = (int64_t)blockIdx.x * RANK_TILE + wv * (64 * RANK_KPT) + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < RANK_KPT; ++k) {
        const int64_t i = base + k * 64;
        ok[k] = i < S;
        key[k] = ok[k] ? src[i] : 0ull;
        const int digit = (int)((key[k] >> shift) & 255ull);
        const unsigned long long peers = rank_peers(digit, ok[k]);
        if (ok[k] && (peers & below) == 0ull) atomicAdd(&wcnt[wv][digit], (unsigned int)__popcll(peers));
    }
    __syncthreads();
    {
        unsigned int o = toff[(p * 256 + tid) * ntiles + blockIdx.x];
#pragma unroll
        for (int v = 0; v < RANK_BS / 64; ++v) {
            const unsigned int c = wcnt[v][tid];
            wcnt[v][tid] = o;
            o += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RANK_KPT; ++k) {
        const int digit = (int)((key[k] >> shift) & 255ull);
        const unsigned long long peers = rank_peers(digit, ok[k]);
        const int lead = ok[k] ? __ffsll(peers) - 1 : lane;
        unsigned int first = 0u;
        if (ok[k] && lane == lead) first = atomicAdd(&wcnt[wv][digit], (unsigned int)__popcll(peers));
        first = (unsigned int)__shfl((int)first, lead);
        const int64_t pos = (int64_t)first + __popcll(peers & below);
        if (ok[k] && pos < S) dst[pos] = key[k];
    }
}

// grid: x = 256 draws, y = parameter.  where[p]: the buffer that holds parameter p's sorted keys.  out: N x d x w.
// mode: DEMCZ_RANK_Z or DEMCZ_RANK_AVERAGE.  A parameter with a NaN in the window is NaN throughout.
__global__ void __launch_bounds__(RANK_BS) rank_score_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t S,
                                                             const double* __restrict__ center, const uint64_t* __restrict__ buf0,
                                                             const uint64_t* __restrict__ buf1, const int* __restrict__ where,
                                                             const unsigned long long* __restrict__ nan_count, int mode,
                                                             double* __restrict__ out)
{
    const int64_t p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * RANK_BS + threadIdx.x;
    if (i >= S) return;
    const bool folded = center != nullptr;
    const int64_t t = i / N, c = i - t * N;
    const double x = chain[c + N * p + N * d * (s0 + t)];
    const uint64_t key = rank_key_of(rank_value_of(x, folded, folded ? center[p] : 0.0));
    const uint64_t* sorted = (where[p] ? buf1 : buf0) + p * S;
    int64_t lo = 0, hi = S;
    while (lo < hi) {                                                    // first index with sorted[index] >= key
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t less = lo;
    // first index with sorted[index] > key: a gallop from `less` (a run of equal keys is short unless the chain stood still), then
    // the bisection of the last step.  Below lo every key is <= key; hi is S or holds a larger key.
    hi = lo;
    for (int64_t step = 1; hi < S && sorted[hi] <= key; step <<= 1) {
        lo = hi + 1;
        hi = (hi + step < S) ? hi + step : S;
    }
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] <= key) lo = mid + 1; else hi = mid;
    }
    const double r = rank_average(less, lo - less);
    double val;
    if (nan_count[p] != 0ull) val = __builtin_nan("");
    else val = (mode == DEMCZ_RANK_AVERAGE) ? r : rank_to_z(r, (double)S);
    out[c + N * p + N * d * t] = val;
}

// One lane per output entry j = c + N (col + m g), m = d nthr columns, col = p + d u; total = N m w entries, strided over.
// thr: [d nthr].  out: N x m x w.
__global__ void __launch_bounds__(256) indicator_le_kernel(const double* __restrict__ chain, int64_t N, int d, int64_t s0, int64_t total,
                                                           int nthr, const double* __restrict__ thr, double* __restrict__ out)
{
    const int64_t m = (int64_t)d * nthr;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
        const int64_t row = j / N, c = j - row * N;
        const int64_t g = row / m, col = row - g * m;
        const int64_t p = col % d;
        const double x = chain[c + N * p + N * d * (s0 + g)];
        out[j] = (x != x) ? x : ((x <= thr[col]) ? 1.0 : 0.0);
    }
}

}  // namespace demcz
