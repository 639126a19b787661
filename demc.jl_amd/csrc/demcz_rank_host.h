// demcz_rank_host.h -- the average rank -> normal score step of the rank-normalised diagnostics, one
// operation sequence for the host and the device: the library's host entry point demcz_rank_to_z, the rank-and-score kernel
// (demcz_kernels_rank.h) and a stand-alone program (tests/c_abi/rank_host_main.cpp) all compile this text.  Plain C++ outside
// hipcc, no HIP calls.
//
//   rl = min(r, S + 1 - r)                      the rank counted from the nearer end (both are multiples of 1/2: exact)
//   u  = (rl - 0.375) / (S + 0.25)              Blom's offsets, one rounded division of two exact operands; 0 < u <= 0.5
//   z  = PPND16(u)                              Wichura's AS 241 (Appl. Statist. 37, 1988), the three rational approximations
//                                               in Horner form in the published order, sqrt(-log(u)) in the outer two
//   z  = -z for r > S + 1 - r
// so that z(S + 1 - r) == -z(r) to the bit and z((S + 1) / 2) == 0.  The logarithm is dm_log (demcz_device.h) on the device
// and the same operation sequence restated here for the host; sqrt is the correctly rounded one on both.  No fma: compile with
// -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/demcz.h"

#if defined(__HIPCC__)
#include "demcz_device.h"
#define DEMCZ_HD __host__ __device__
#else
#define DEMCZ_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace demcz {

// dm_log's operation sequence (fdlibm's log for a positive normal argument) for the host
inline double rank_log_host(double x)
{
    const double LN2_HI = 6.93147180369123816490e-01;
    const double LN2_LO = 1.90821492927058770002e-10;
    const double LG1 = 6.666666666666735130e-01;
    const double LG2 = 3.999999999940941908e-01;
    const double LG3 = 2.857142874366239149e-01;
    const double LG4 = 2.222219843214978396e-01;
    const double LG5 = 1.818357216161805012e-01;
    const double LG6 = 1.531383769920937332e-01;
    const double LG7 = 1.479819860511658591e-01;
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    uint32_t hx = (uint32_t)(b >> 32);
    const uint32_t lx = (uint32_t)b;
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    const uint64_t rb = ((uint64_t)hx << 32) | lx;
    double xr;
    std::memcpy(&xr, &rb, sizeof xr);
    const double f = xr - 1.0;
    const double hfsq = (0.5 * f) * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (LG2 + w * (LG4 + w * LG6));
    const double t2 = z * (LG1 + w * (LG3 + w * (LG5 + w * LG7)));
    const double R = t2 + t1;
    const double dk = (double)k;
    return ((((s * (hfsq + R)) + (dk * LN2_LO)) - hfsq) + f) + (dk * LN2_HI);
}

DEMCZ_HD inline double rank_log(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return dm_log(x);
#else
    return rank_log_host(x);
#endif
}

// AS 241 PPND16 for 0 < u <= 0.5: the normal quantile of the lower half (<= 0)
DEMCZ_HD inline double rank_ppnd16_lower(double u)
{
    const double q = u - 0.5;
    if (q >= -0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r + 67265.770927008700853) * r
                                + 45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r
                             + 133.14166789178437745) * r + 3.387132872796366608);
        const double den = (((((((5226.495278852854561 * r + 28729.085735721942674) * r + 39307.89580009271061) * r
                                + 21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r
                             + 42.313330701600911252) * r + 1.0);
        return (q * num) / den;
    }
    const double lg = rank_log(u);
    double r = std::sqrt(-lg);
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r + 0.24178072517745061177) * r
                   + 1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r
                + 4.6303378461565452959) * r + 1.42343711074968357734);
        den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r
                   + 0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r
                + 2.05319162663775882187) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r
                   + 0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r
                + 5.4637849111641143699) * r + 6.6579046435011037772);
        den = (((((((2.04426310338993978564e-15 * r + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r
                   + 7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r
                + 0.59983220655588793769) * r + 1.0);
    }
    return -(num / den);
}

// r: an average rank in [1, S] (a multiple of 1/2 when it comes from counts); S >= 1 draws
DEMCZ_HD inline double rank_to_z(double r, double S)
{
    const double mirror = (S + 1.0) - r;
    const bool upper = r > mirror;
    const double rl = upper ? mirror : r;
    const double u = (rl - 0.375) / (S + 0.25);
    const double z = rank_ppnd16_lower(u);
    return upper ? -z : z;
}

// the average rank from the two counts: less + (equal + 1) / 2, exact
DEMCZ_HD inline double rank_average(int64_t less, int64_t equal)
{
    return (double)less + 0.5 * (double)(equal + 1);
}

}  // namespace demcz

// z[i] = the normal score of average rank r[i] among S draws.  Host code, no device.  1 <= r[i] <= S, S < 2^50.
extern "C" int32_t demcz_rank_to_z(int64_t n, const double* r, int64_t S, double* z)
{
    if (n < 0 || S < 1 || S >= ((int64_t)1 << 50) || (n > 0 && (!r || !z))) return DEMCZ_ERR_INVALID_ARGUMENT;
    const double dS = (double)S;
    for (int64_t i = 0; i < n; ++i)
        if (!(r[i] >= 1.0 && r[i] <= dS)) return DEMCZ_ERR_INVALID_ARGUMENT;                 // (a NaN fails both comparisons)
    for (int64_t i = 0; i < n; ++i) z[i] = demcz::rank_to_z(r[i], dS);
    return DEMCZ_OK;
}
