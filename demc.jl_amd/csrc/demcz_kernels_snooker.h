// demcz_kernels_snooker.h -- the snooker update of DE-MCzs (ter Braak & Vrugt 2008) for gfx950: ONE generation in which every
// chain jumps along the line from an anchor row of the archive through its own state, by the difference of two other rows
// projected onto that line ("snooker generations", and section 4.15).
//
//   snooker_kernel<TARGET, D>        compile-time D: state, rows and proposal in registers
//   snooker_kernel_generic<TARGET>   run-time d <= MAX_D: state and proposal in LDS, one column per lane
//
// Both take the WindowParams of window_kernel and carry its duties for ngen == 1 (state in and out, history slot, append / snap
// at a K boundary, the ballot counts), so that everything behind a window launch works on a snooker launch as it is.  One lane
// per chain.  The step spans all d parameters whatever the handle's blocks are and replaces the generation's block-steps.
// No fma anywhere in the step: every product and sum is rounded on its own (tests/snooker_reference.py is plain Python floats).
#pragma once

#include "demcz_kernels.h"

#pragma clang fp contract(off)

namespace demcz {

// what a snooker launch is told beside WindowParams (a second kernel argument: WindowParams stays the struct it is)
struct SnookerParams {
    double gamma_lo, gamma_hi;       // gamma_s ~ U(gamma_lo, gamma_hi)
};

// The third row: uniform over the M - 2 rows that are neither i1 nor i2.
__device__ __forceinline__ uint64_t draw_anchor(uint64_t r1, uint64_t M, uint64_t i1, uint64_t i2)
{
    uint64_t j = (M <= 0xffffffffull) ? mulhi64_u32(r1, (uint32_t)(M - 2)) : __umul64hi(r1, M - 2);      // wave-uniform choice
    const uint64_t lo = (i1 < i2) ? i1 : i2, hi = (i1 < i2) ? i2 : i1;
    if (j >= lo) ++j;
    if (j >= hi) ++j;
    return j;
}

// e2 / f2 of a step that may be taken: finite positive normal doubles, the domain of dm_log
__device__ __forceinline__ bool snooker_norm_ok(double v) { return v >= 0x1p-1022 && v <= 0x1.fffffffffffffp+1023; }

// accept test of the step; the Jacobian (|xp - a| / |x - a|)^(d-1) is geometry and is not tempered
__device__ __forceinline__ bool snooker_accept(const WindowParams& P, int d, double e2, double f2, double lpp, double lp, double logu)
{
    const double jac = (0.5 * (double)(d - 1)) * (dm_log(f2) - dm_log(e2));
    double dlt = lpp - lp;
    if (P.temperature) dlt = dlt / P.temperature[0];
    const bool valid = snooker_norm_ok(e2) && snooker_norm_ok(f2);
    return valid && logu < dlt + jac;
}

template <int TARGET, int D>
__global__ void __launch_bounds__(WINDOW_BS) snooker_kernel(const WindowParams P, const SnookerParams SP)
{
    const int64_t c = (int64_t)blockIdx.x * WINDOW_BS + threadIdx.x;
    if (c >= P.N) return;

    double x[D];
#pragma unroll
    for (int p = 0; p < D; ++p) x[p] = P.Xcur[c + P.N * p];
    double lp = P.lpcur[c];
    // target constants in scalar registers where window_kernel keeps them there
    constexpr bool LOCAL_TARGET = (TARGET == TARGET_MVNORMAL && D <= 10) || TARGET == TARGET_ISO_QUAD;
    [[maybe_unused]] double muc[LOCAL_TARGET ? D : 1], Wc[(LOCAL_TARGET && TARGET == TARGET_MVNORMAL) ? D * (D + 1) / 2 : 1];
    if constexpr (LOCAL_TARGET) {
#pragma unroll
        for (int p = 0; p < D; ++p) muc[p] = uniform_double(P.tp.mu[p]);
        if constexpr (TARGET == TARGET_MVNORMAL) {
#pragma unroll
            for (int i = 0; i < D * (D + 1) / 2; ++i) Wc[i] = uniform_double(P.tp.Wp[i]);
        }
    }
    [[maybe_unused]] const double c0c = P.tp.c0;
    // the log-density of a point: the operation sequence of target_logp (grouped by the handle's blocks where those group it)
    auto logp_of = [&](const double (&xq)[D]) -> double {
        if constexpr (TARGET == TARGET_MVNORMAL) {
            if (P.tp.ngrp > 1) return target_logp<TARGET, D>(P.tp, D, [&](int j) { return xq[j]; });
        }
        if constexpr (LOCAL_TARGET && TARGET == TARGET_MVNORMAL) {
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double acc = Wc[(i * (i + 1)) / 2] * (xq[0] - muc[0]);
#pragma unroll
                for (int j = 1; j <= i; ++j) acc = fma(Wc[(i * (i + 1)) / 2 + j], xq[j] - muc[j], acc);
                q = (i == 0) ? acc * acc : fma(acc, acc, q);
            }
            return fma(-0.5, q, c0c);
        } else if constexpr (LOCAL_TARGET) {
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double rr = xq[i] - muc[i];
                q = (i == 0) ? rr * rr : fma(rr, rr, q);
            }
            return -q;
        } else {
            return target_logp<TARGET, D>(P.tp, D, [&](int j) { return xq[j]; });
        }
    };

    rng_state st;
    rng_seek(st, P.seed, (uint64_t)(P.chain_id0 + c), (uint64_t)(P.g_first - 1) * (uint64_t)P.S);
    const unsigned long long speak64 = __builtin_amdgcn_ballot_w64(true);      // every lane still here runs a chain

    uint64_t r1, r2, i1, i2;
    rng_next(st, r1, r2);
    draw_rows(r1, r2, (uint64_t)P.M, i1, i2);
    uint64_t q1, q2;
    rng_next(st, q1, q2);
    const uint64_t ia = draw_anchor(q1, (uint64_t)P.M, i1, i2);
    // the three rows are asked for as soon as their indices exist, in front of the arithmetic of gamma_s and log u.  (The
    // optimiser sinks log u's part of it down to the accept test, its only use; holding it here measured the same: DESIGN.md 4.15)
    double a[D], z1[D], z2[D];
    load_row<D>(P.Z + (int64_t)ia * P.ZS, a);
    load_row<D>(P.Z + (int64_t)i1 * P.ZS, z1);
    load_row<D>(P.Z + (int64_t)i2 * P.ZS, z2);
    __builtin_amdgcn_sched_barrier(0);
    const double gspan = SP.gamma_hi - SP.gamma_lo;
    const double gprod = gspan * u_open(q2);
    const double gs = SP.gamma_lo + gprod;
    rng_next(st, r1, r2);
    const double logu = dm_log(u_open(r1));

    double e[D];
    double e2 = 0.0, t = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        e[p] = x[p] - a[p];
        const double ee = e[p] * e[p];
        const double dz = z1[p] - z2[p];
        const double te = dz * e[p];
        e2 = (p == 0) ? ee : e2 + ee;
        t = (p == 0) ? te : t + te;
    }
    const double cc = gs * (t / e2);
    double xp[D];
    double f2 = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        const double step = cc * e[p];
        xp[p] = x[p] + step;
        const double f = xp[p] - a[p];
        const double ff = f * f;
        f2 = (p == 0) ? ff : f2 + ff;
    }
    const double lpp = logp_of(xp);
    const bool acc = snooker_accept(P, D, e2, f2, lpp, lp, logu);
    const double lp0 = lp;
#pragma unroll
    for (int p = 0; p < D; ++p) x[p] = acc ? xp[p] : x[p];
    lp = acc ? lpp : lp;

    const unsigned int k = wave_count_changed(lp, lp0, speak64);
    if (P.chain) {
#pragma unroll
        for (int p = 0; p < D; ++p) P.chain[c + P.N * (p + (int64_t)D * P.slot_first)] = x[p];
        P.logobj[c + P.N * P.slot_first] = lp;
    }
    if (P.to_boundary == 1) {                  // the generation is a multiple of K: the append of any generation
        if (P.do_append) store_row<D>(P.Zw + (P.M_append + c) * P.ZS, x);
        if (P.snap) {
#pragma unroll
            for (int p = 0; p < D; ++p) P.snap[c + P.N * p] = x[p];
        }
    }
#pragma unroll
    for (int p = 0; p < D; ++p) P.Xcur[c + P.N * p] = x[p];
    P.lpcur[c] = lp;
    wave_store_counts(P, blockIdx.x, k, k);
}

// run-time d: x and the proposal in LDS (2 d columns of WINDOW_BS doubles, dynamic), the rows read where they are used
template <int TARGET>
__global__ void __launch_bounds__(WINDOW_BS) snooker_kernel_generic(const WindowParams P, const SnookerParams SP)
{
    extern __shared__ double lds[];
    const int d = P.d;
    double* xs = lds;                         // d x BS
    double* xps = lds + d * WINDOW_BS;        // d x BS
    const int64_t c = (int64_t)blockIdx.x * WINDOW_BS + threadIdx.x;
    if (c >= P.N) return;
    const int tid = threadIdx.x;

    double lp = P.lpcur[c];
    rng_state st;
    rng_seek(st, P.seed, (uint64_t)(P.chain_id0 + c), (uint64_t)(P.g_first - 1) * (uint64_t)P.S);
    const unsigned long long speak64 = __builtin_amdgcn_ballot_w64(true);

    uint64_t r1, r2, i1, i2;
    rng_next(st, r1, r2);
    draw_rows(r1, r2, (uint64_t)P.M, i1, i2);
    uint64_t q1, q2;
    rng_next(st, q1, q2);
    const uint64_t ia = draw_anchor(q1, (uint64_t)P.M, i1, i2);
    const double* za = P.Z + (int64_t)ia * P.ZS;
    const double* zb1 = P.Z + (int64_t)i1 * P.ZS;
    const double* zb2 = P.Z + (int64_t)i2 * P.ZS;
    double e2 = 0.0, t = 0.0;
    for (int p = 0; p < d; ++p) {
        const double xv = P.Xcur[c + P.N * p];
        xs[p * WINDOW_BS + tid] = xv;
        const double ev = xv - za[p];
        const double ee = ev * ev;
        const double dz = zb1[p] - zb2[p];
        const double te = dz * ev;
        e2 = (p == 0) ? ee : e2 + ee;
        t = (p == 0) ? te : t + te;
    }
    const double gspan = SP.gamma_hi - SP.gamma_lo;
    const double gprod = gspan * u_open(q2);
    const double gs = SP.gamma_lo + gprod;
    rng_next(st, r1, r2);
    const double logu = dm_log(u_open(r1));
    const double cc = gs * (t / e2);
    double f2 = 0.0;
    for (int p = 0; p < d; ++p) {
        const double xv = xs[p * WINDOW_BS + tid];
        const double av = za[p];
        const double ev = xv - av;
        const double step = cc * ev;
        const double xpv = xv + step;
        xps[p * WINDOW_BS + tid] = xpv;
        const double f = xpv - av;
        const double ff = f * f;
        f2 = (p == 0) ? ff : f2 + ff;
    }
    const double lpp = target_logp<TARGET, 0>(P.tp, d, [&](int j) { return xps[j * WINDOW_BS + tid]; });
    const bool acc = snooker_accept(P, d, e2, f2, lpp, lp, logu);
    const double lp0 = lp;
    lp = acc ? lpp : lp;
    const double* xfin = acc ? xps : xs;      // the column the chain's state is in now

    const unsigned int k = wave_count_changed(lp, lp0, speak64);
    const bool boundary = P.to_boundary == 1;
    for (int p = 0; p < d; ++p) {
        const double xv = xfin[p * WINDOW_BS + tid];
        if (P.chain) P.chain[c + P.N * (p + (int64_t)d * P.slot_first)] = xv;
        if (boundary && P.do_append) P.Zw[(P.M_append + c) * P.ZS + p] = xv;
        if (boundary && P.snap) P.snap[c + P.N * p] = xv;
        P.Xcur[c + P.N * p] = xv;
    }
    if (P.chain) P.logobj[c + P.N * P.slot_first] = lp;
    P.lpcur[c] = lp;
    wave_store_counts(P, blockIdx.x, k, k);
}

#ifndef DEMCZ_PROGRAM_TARGET
// the built-in instantiations live in demcz_snooker_inst.hip; this hands out their host symbols.  *dyn_lds: dynamic LDS bytes of
// the launch (the run-time-d form).  nullptr: no built-in kernel for that target (program targets bring their own).
const void* snooker_kernel_fn(int target_kind, int d, size_t* dyn_lds);
#endif

}  // namespace demcz
