// demcz_loo_host.h -- the host half of PSIS-LOO and WAIC (DESIGN.md sections 3 and 4.16): the per-term functions of the
// generalised-Pareto tail fit (Zhang & Stephens 2009, as used by Vehtari, Gelman & Gabry 2017 and Vehtari, Simpson, Gelman, Yao
// & Gabry 2024), one text for the host and the device, a serial fit built from them (demcz_gpd_fit), the tail length
// (demcz_psis_tail_length) and the chunk planner of demcz_loo.  The fit kernel (demcz_kernels_loo.h) and a stand-alone program
// (tests/c_abi/loo_host_main.cpp) both compile this text.  Plain C++ outside hipcc, no HIP calls.
//
// With lw_j = a_0 - a_j the log importance ratios of one observation, largest first (a: its log-likelihoods, ascending):
//   M     = ceil(min(S / 5, 3 sqrt(S / r_eff)))                                    (and at most S - 1: the index must exist)
//   c     = max(lw_M, log DBL_MIN), the tail the n elements with lw > c, strictly
//   x_i   = exp(lw) - exp(c) over the tail, ascending: x_1 <= ... <= x_n
//   b_j   = 1 / x_n + (1 - sqrt(m / (j - 1/2))) / (3 x_q),  j = 1..m = 30 + floor(sqrt(n)),  q = floor(n / 4 + 1/2)
//   k_j   = mean log1p(-b_j x),  L_j = n (log(-b_j / k_j) - k_j - 1),  w_j = 1 / sum_l exp(L_l - L_j)
//   b     = sum b_j w_j,  k = mean log1p(-b x),  sigma = -k / b,  khat = (n k + 5) / (n + 10)
//   the tail's j-th smallest weight becomes min(0, log(sigma expm1(-k log1p(-p_j)) / k + exp(c))),  p_j = (j - 1/2) / n
// The kernel adds the means in its own fixed order (lane-strided partials, a butterfly, the four waves in order); demcz_gpd_fit
// adds them in index order.  No fma: compile with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/demcz.h"

#if defined(__HIPCC__)
#define DEMCZ_LOO_HD __host__ __device__
#else
#define DEMCZ_LOO_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace demcz {

constexpr double LOO_LOG_DBL_MIN = -708.3964185322641;      // log(2.2250738585072014e-308)
constexpr int LOO_MIN_FIT = 5;                              // a tail of fewer elements is not smoothed: khat = +inf
constexpr int LOO_MAX_CAND = 512;                           // candidates of a fit at the most: 30 + floor(sqrt(3 sqrt(2^31))) = 402

// the chunk planner of demcz_loo: an N x mc x w history of log-likelihoods and the sort's two key buffers are 24 mc bytes per draw
constexpr int LOO_MAX_CHUNK = 32;                           // (= DERIVE_MAX_M: what a derived history of a program holds)
constexpr int64_t LOO_BYTES_PER_DRAW_COLUMN = 24;
constexpr int64_t LOO_SCRATCH_BUDGET = (int64_t)4 << 30;    // bytes of device memory demcz_loo lets one chunk take

// M of S draws; r_eff in (0, inf)
DEMCZ_LOO_HD inline int64_t psis_tail_cap(int64_t S, double r_eff)
{
    const double fifth = (double)S / 5.0;
    const double root = 3.0 * std::sqrt((double)S / r_eff);
    const double m = std::ceil(fifth < root ? fifth : root);
    int64_t M = (m < (double)S) ? (int64_t)m : S;
    if (M > S - 1) M = S - 1;
    return M < 0 ? 0 : M;
}

DEMCZ_LOO_HD inline int psis_candidates(int64_t n) { return 30 + (int)std::floor(std::sqrt((double)n)); }

// q, 1-based
DEMCZ_LOO_HD inline int64_t psis_quartile(int64_t n) { return (int64_t)std::floor((double)n / 4.0 + 0.5); }

// b_j, j = 1..m
DEMCZ_LOO_HD inline double gpd_b(int j, int m, double xn, double xq)
{
    return 1.0 / xn + (1.0 - std::sqrt((double)m / ((double)j - 0.5))) / (3.0 * xq);
}

// one term of k_j's mean
DEMCZ_LOO_HD inline double gpd_term(double b, double x) { return std::log1p(-(b * x)); }

// L_j
DEMCZ_LOO_HD inline double gpd_profile(int64_t n, double b, double k) { return (double)n * ((std::log(-(b / k)) - k) - 1.0); }

DEMCZ_LOO_HD inline double gpd_khat(int64_t n, double k) { return ((double)n * k + 5.0) / ((double)n + 10.0); }

// the smoothed log weight of the tail's j-th smallest element, j = 1..n
DEMCZ_LOO_HD inline double psis_smoothed(int64_t j, int64_t n, double k, double sigma, double expc)
{
    const double p = ((double)j - 0.5) / (double)n;
    const double lp = std::log1p(-p);
    const double q = (k == 0.0) ? -(sigma * lp) : (sigma * std::expm1(-(k * lp))) / k;
    const double v = std::log(q + expc);
    return v < 0.0 ? v : 0.0;
}

// the widest chunk of observations whose scratch fits `budget` bytes over S draws: 1..LOO_MAX_CHUNK (1 even where that does not
// fit: the allocation then fails and says so)
inline int loo_chunk_width(int64_t S, int64_t budget)
{
    if (S < 1 || budget < 1) return 1;
    const int64_t per_column = (S > INT64_MAX / LOO_BYTES_PER_DRAW_COLUMN) ? INT64_MAX : S * LOO_BYTES_PER_DRAW_COLUMN;
    const int64_t mc = budget / per_column;
    return mc < 1 ? 1 : (mc > LOO_MAX_CHUNK ? LOO_MAX_CHUNK : (int)mc);
}

// chunk i of nobs observations in chunks of mc: its first observation and its width (0 past the end)
inline void loo_chunk(int64_t nobs, int mc, int64_t i, int64_t* from, int* count)
{
    *from = (i < 0 || mc < 1 || i > nobs / mc) ? nobs : i * mc;
    if (*from > nobs) *from = nobs;
    const int64_t left = nobs - *from;
    *count = (int)(left < mc ? (left < 0 ? 0 : left) : mc);
}

inline int64_t loo_chunk_count(int64_t nobs, int mc) { return (nobs < 1 || mc < 1) ? 0 : (nobs + mc - 1) / mc; }

}  // namespace demcz

// *M = the tail length the fit starts from: host code, no device.
extern "C" int32_t demcz_psis_tail_length(int64_t S, double r_eff, int64_t* M)
{
    if (!M || S < 1 || !(r_eff > 0.0) || !(r_eff < INFINITY)) return DEMCZ_ERR_INVALID_ARGUMENT;
    *M = demcz::psis_tail_cap(S, r_eff);
    return DEMCZ_OK;
}

// The fit of n >= 5 exceedances x_1 <= ... <= x_n (positive): k and sigma of the generalised Pareto distribution and the
// regularised khat.  Host code, no device; sums in index order.  Any output may be NULL.
extern "C" int32_t demcz_gpd_fit(int64_t n, const double* x_ascending, double* k, double* sigma, double* khat)
{
    if (n < demcz::LOO_MIN_FIT || !x_ascending) return DEMCZ_ERR_INVALID_ARGUMENT;
    const int m = demcz::psis_candidates(n);
    if (m > demcz::LOO_MAX_CAND) return DEMCZ_ERR_INVALID_ARGUMENT;
    const double* x = x_ascending;
    const double xn = x[n - 1], xq = x[demcz::psis_quartile(n) - 1];
    double b[demcz::LOO_MAX_CAND], L[demcz::LOO_MAX_CAND];
    for (int j = 1; j <= m; ++j) {
        const double bj = demcz::gpd_b(j, m, xn, xq);
        double s = 0.0;
        for (int64_t i = 0; i < n; ++i) s += demcz::gpd_term(bj, x[i]);
        b[j - 1] = bj;
        L[j - 1] = demcz::gpd_profile(n, bj, s / (double)n);
    }
    double bhat = 0.0;
    for (int j = 0; j < m; ++j) {
        double s = 0.0;
        for (int l = 0; l < m; ++l) s += std::exp(L[l] - L[j]);
        bhat += b[j] * (1.0 / s);
    }
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += demcz::gpd_term(bhat, x[i]);
    const double kk = s / (double)n;
    if (k) *k = kk;
    if (sigma) *sigma = -(kk / bhat);
    if (khat) *khat = demcz::gpd_khat(n, kk);
    return DEMCZ_OK;
}
