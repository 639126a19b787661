// demcz_select_host.h -- the host half of the quantile selection: plain C++, no HIP calls, so that it also
// builds into a stand-alone program (tests/c_abi/select_host_main.cpp).  The device half (demcz_kernels_sel.h) counts, per
// parameter and key prefix, the draws by one byte of their order-preserving key; the three functions here turn a probability
// into ranks, walk a rank one byte down the key from those counts, and turn the two order statistics into the quantile.
//
//   key(x) = bits(x) ^ 0xFFFF...F  when the sign bit is set, bits(x) | 1 << 63  otherwise:
//   -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN  as unsigned integers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/demcz.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace demcz {

constexpr int SEL_MAX_PROBS = 16;                     // probabilities per call
constexpr int SEL_MAX_PREFIX = 2 * SEL_MAX_PROBS;     // ranks per parameter, and so distinct prefixes per parameter and pass

inline uint64_t sel_key_of_bits(uint64_t b) { return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63)); }
inline uint64_t sel_bits_of_key(uint64_t k) { return (k >> 63) ? (k ^ ((uint64_t)1 << 63)) : ~k; }
inline double sel_double_of_key(uint64_t k)
{
    const uint64_t b = sel_bits_of_key(k);
    double x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

}  // namespace demcz

// Hyndman-Fan type 7: h = (S - 1) q, rank_lo = floor(h) clipped to [0, S-1], rank_hi = min(rank_lo + 1, S - 1), frac = h - rank_lo.
extern "C" int32_t demcz_quantile_plan(int64_t S, int32_t nq, const double* probs, int64_t* rank_lo, int64_t* rank_hi, double* frac)
{
    if (S < 1 || nq < 1 || nq > demcz::SEL_MAX_PROBS || !probs || !rank_lo || !rank_hi || !frac) return DEMCZ_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < nq; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return DEMCZ_ERR_INVALID_ARGUMENT;        // (a NaN fails both comparisons)
    for (int j = 0; j < nq; ++j) {
        const double h = (double)(S - 1) * probs[j];
        int64_t lo = (int64_t)std::floor(h);
        if (lo < 0) lo = 0;
        if (lo > S - 1) lo = S - 1;
        rank_lo[j] = lo;
        rank_hi[j] = (lo + 1 < S - 1) ? lo + 1 : S - 1;
        frac[j] = h - (double)lo;
    }
    return DEMCZ_OK;
}

// One byte of the walk: counts[b + 256 (r + nr p)] = draws of parameter p whose key starts with prefix[p + d r] and goes on with
// byte b (added over the shards by the caller).  rank[p + d r] is the 0-based rank among the draws that share the prefix.
extern "C" int32_t demcz_select_step(int32_t d, int32_t nr, const int64_t* counts, uint64_t* prefix, int64_t* rank)
{
    if (d < 1 || nr < 1 || !counts || !prefix || !rank) return DEMCZ_ERR_INVALID_ARGUMENT;
    for (int p = 0; p < d; ++p)                    // nothing is written unless every rank can be placed
        for (int r = 0; r < nr; ++r) {
            const int64_t* c = counts + 256 * ((size_t)r + (size_t)nr * p);
            const int64_t k = rank[p + (size_t)d * r];
            int64_t total = 0;
            for (int b = 0; b < 256; ++b) {
                if (c[b] < 0 || total > INT64_MAX - c[b]) return DEMCZ_ERR_INVALID_ARGUMENT;
                total += c[b];
            }
            if (k < 0 || k >= total) return DEMCZ_ERR_INVALID_ARGUMENT;
        }
    for (int p = 0; p < d; ++p)
        for (int r = 0; r < nr; ++r) {
            const int64_t* c = counts + 256 * ((size_t)r + (size_t)nr * p);
            int64_t k = rank[p + (size_t)d * r];
            int b = 0;
            while (k >= c[b]) k -= c[b++];         // (k < total: b stays below 256)
            rank[p + (size_t)d * r] = k;
            prefix[p + (size_t)d * r] = (prefix[p + (size_t)d * r] << 8) | (uint64_t)b;
        }
    return DEMCZ_OK;
}

// a = x_(lo), b = x_(hi) from their keys; q = a when frac == 0 or a == b, else a + frac (b - a), each operation rounded.
// A parameter with nan_count[p] != 0 is NaN in q, lower and upper.  nan_count, lower and upper may be NULL.
extern "C" int32_t demcz_quantile_finish(int32_t d, int32_t nq, const uint64_t* key_lo, const uint64_t* key_hi, const double* frac,
                                         const int64_t* nan_count, double* q, double* lower, double* upper)
{
    if (d < 1 || nq < 1 || nq > demcz::SEL_MAX_PROBS || !key_lo || !key_hi || !frac || !q) return DEMCZ_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < nq; ++j)
        for (int p = 0; p < d; ++p) {
            const size_t i = p + (size_t)d * j;
            double a = demcz::sel_double_of_key(key_lo[i]), b = demcz::sel_double_of_key(key_hi[i]), v;
            if (nan_count && nan_count[p] != 0) {
                a = b = v = std::nan("");
            } else if (frac[j] == 0.0 || a == b) {
                v = a;
            } else {
                const double diff = b - a;
                const double step = frac[j] * diff;
                v = a + step;
            }
            q[i] = v;
            if (lower) lower[i] = a;
            if (upper) upper[i] = b;
        }
    return DEMCZ_OK;
}
