// demcz_kernels_crossover.h -- crossover generations of DREAM(ZS) (Vrugt et al. 2009; Laloy & Vrugt 2012) for gfx950: every
// chain moves a random subset of its parameters by the sum of delta archive differences, ONE step and ONE log-density evaluation
// per generation ("crossover generations", and section 4.20).
//
//   window_kernel_cr<TARGET, D>        compile-time D: state, proposal and the running difference sum in registers
//   window_kernel_cr_generic<TARGET>   run-time d <= MAX_D: state and proposal in LDS, one column per lane, rows read where used
//
// Both take the WindowParams of window_kernel<T, D, true> and carry all its duties (any ngen, the countdown to the K boundary with
// do_append / snap, history slots, state in and out, the ballot counts, temperature[gi]), so that everything behind a window
// launch works on a crossover launch as it is.  What is new travels in a second kernel argument, CrossoverParams.  One lane per
// chain.  The CR class, the number of pairs and the subset differ from lane to lane: the subset is a 64-bit lane-local mask applied
// with selects, the gathers of pair j are predicated on j <= delta.  No fma in the proposal: every product and sum is rounded on
// its own (tests/crossover_reference.py is plain Python floats).
//
//   window_kernel_cr<TARGET, D, true>, window_kernel_cr_generic<TARGET, true>   the same generations with the class weights adapted
//       during burn-in (demcz_set_crossover_adapt): a third kernel argument, CrossoverAdaptParams, brings the cumulative weights
//       from DEVICE memory -- they change between launches with no host in between -- and, while `accumulate` is set, every
//       accepted step's squared jump distance, normalised by the population's spread and quantised to an integer, is added up per
//       class (tests/crossover_adapt_reference.py).  The two-argument kernels are what they were: both forms are one body,
//       and everything of the adaptation in it is behind `if constexpr (ADAPT)`.
//   cr_adapt_kernel   the update behind the launch that ends on an update position: the new weights from jump distance per
//       step tried, and the spread (rsd) of the chains as they stand.
#pragma once

#include "demcz_kernels.h"

#pragma clang fp contract(off)

namespace demcz {

constexpr int CR_MAX_CLASSES = 8;
constexpr int CR_MAX_PAIRS = 3;

// what a crossover launch is told beside WindowParams (a second kernel argument: WindowParams stays the struct it is)
struct CrossoverParams {
    int32_t ncr;                           // CR classes, 1..8: class m selects a parameter with probability (m + 1) / ncr
    int32_t delta_max;                     // 1..3: delta ~ U{1..delta_max} difference pairs
    uint32_t cum[CR_MAX_CLASSES];          // cum[k] = w_0 + ... + w_k for k < ncr, W = cum[ncr - 1] for k >= ncr
    unsigned long long* counts;            // [workgroup][8][2]: steps tried and accepted per class, summed over the handle's life
};

// what an ADAPT launch is told beside that (a third kernel argument: WindowParams and CrossoverParams stay the structs they are)
struct CrossoverAdaptParams {
    const uint32_t* cum;                   // [8] in device memory, laid out as CrossoverParams::cum: read once at launch start
    const double* rsd;                     // [d]: reciprocal standard deviation of every parameter over the chains (0: the column does not count)
    unsigned long long* slots;             // [workgroup][8][2]: quantised jump distance and steps tried per class, while adaptation runs
    int32_t accumulate;                    // launch-uniform: the launch lies at or in front of `until`
};

// q of an accepted step with squared normalised jump distance J: 16.16 fixed point, clamped at 65536; NaN and negatives give 0
__device__ __forceinline__ unsigned long long cr_quantise(double J)
{
    const double Jc = (J < 65536.0) ? J : 65536.0;
    const double sc = Jc * 65536.0;
    return (J >= 0.0) ? (unsigned long long)sc : 0ull;
}

// Per-class sums of q of a lane: eight predicated adds a step (no dynamically indexed register array), reduced over the wave at the
// end of the launch.  The lanes that run a chain are lanes 0 .. nact - 1; what a shuffle reads from a lane beyond them is not used.
struct CrDist {
    unsigned long long q[CR_MAX_CLASSES];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) q[k] = 0ull;
    }
    __device__ __forceinline__ void add(int m, unsigned long long v)
    {
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) q[k] += (m == k) ? v : 0ull;
    }
    // lane 0 adds the wave's sums and the steps tried into the workgroup's own sixteen slots (plain loads and stores, as
    // CrCounts::add_to does)
    __device__ __forceinline__ void add_to(unsigned long long* slots, const unsigned int (&tried)[CR_MAX_CLASSES], int nact)
    {
        const int lane = (int)threadIdx.x;
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
#pragma unroll
            for (int sft = 32; sft >= 1; sft >>= 1) {
                const unsigned long long o = __shfl_down(q[k], sft, 64);
                q[k] += (lane + sft < nact) ? o : 0ull;
            }
        }
        if (lane != 0) return;
        unsigned long long* slot = slots + (size_t)blockIdx.x * (2 * CR_MAX_CLASSES);
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            slot[2 * k] = slot[2 * k] + q[k];
            slot[2 * k + 1] = slot[2 * k + 1] + (unsigned long long)tried[k];
        }
    }
};

// the one element of an ADAPT kernel's trailing arguments
__device__ __forceinline__ const CrossoverAdaptParams& cr_adapt_params(const CrossoverAdaptParams& A) { return A; }
// C with the cumulative weights read from device memory (uniform loads, once a launch)
__device__ __forceinline__ CrossoverParams cr_adapted(const CrossoverParams& C, const CrossoverAdaptParams& A)
{
    CrossoverParams Cl;
    Cl.ncr = C.ncr;
    Cl.delta_max = C.delta_max;
    Cl.counts = C.counts;
#pragma unroll
    for (int k = 0; k < CR_MAX_CLASSES; ++k) Cl.cum[k] = A.cum[k];
    return Cl;
}

// Philox blocks of a crossover generation: choices, delta_max pairs, ceil(d / 4) of subset words, ceil(d / 2) of normals, log u
__host__ __device__ constexpr int64_t crossover_stride(int d, int delta_max) { return 1 + delta_max + (d + 3) / 4 + (d + 1) / 2 + 1; }

// The choices of block B.  m: the smallest k with j < cum[k], j = (hi32(r1) W) >> 32 < W -- the number of k with cum[k] <= j.
__device__ __forceinline__ void cr_choices(const CrossoverParams& C, uint64_t r1, uint64_t r2, int d, int& m, int& delta, int& pstar)
{
    const uint32_t lo = (uint32_t)r1, hi = (uint32_t)(r1 >> 32);
    const uint32_t j = (uint32_t)(((uint64_t)hi * (uint64_t)C.cum[CR_MAX_CLASSES - 1]) >> 32);
    int mm = 0;
#pragma unroll
    for (int k = 0; k < CR_MAX_CLASSES - 1; ++k) mm += (j >= C.cum[k]) ? 1 : 0;
    m = mm;
    delta = 1 + (int)(((uint64_t)lo * (uint64_t)(uint32_t)C.delta_max) >> 32);
    pstar = (int)mulhi64_u32(r2, (uint32_t)d);
}

// word selects its parameter in class m: (uint64) word * ncr < (uint64)(m + 1) << 32
__device__ __forceinline__ bool cr_selects(uint32_t word, int ncr, int m)
{
    return (uint64_t)word * (uint64_t)(uint32_t)ncr < ((uint64_t)(uint32_t)(m + 1) << 32);
}

// Per-class counts of a wave, in scalar registers: ballots of the lanes in class k, and of those whose accept test was true.
struct CrCounts {
    unsigned int tried[CR_MAX_CLASSES], accepted[CR_MAX_CLASSES];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) tried[k] = accepted[k] = 0u;
    }
    __device__ __forceinline__ void count(int ncr, int m, bool acc, unsigned long long speak64)
    {
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            if (k < ncr) {                      // wave-uniform
                const unsigned long long in_k = __builtin_amdgcn_ballot_w64(m == k) & speak64;
                const unsigned long long acc_k = __builtin_amdgcn_ballot_w64(m == k && acc) & speak64;
                tried[k] += (unsigned int)__builtin_popcountll(in_k);
                accepted[k] += (unsigned int)__builtin_popcountll(acc_k);
            }
        }
    }
    // lane 0 (it always runs a chain) adds the counts into the workgroup's own sixteen slots: a workgroup always runs the same
    // chains and launches on a stream are ordered, so plain loads and stores do
    __device__ __forceinline__ void add_to(unsigned long long* counts) const
    {
        if (!counts || threadIdx.x != 0) return;
        unsigned long long* slot = counts + (size_t)blockIdx.x * (2 * CR_MAX_CLASSES);
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            slot[2 * k] = slot[2 * k] + (unsigned long long)tried[k];
            slot[2 * k + 1] = slot[2 * k + 1] + (unsigned long long)accepted[k];
        }
    }
};

// rows in flight: all 2 delta_max rows are asked for in front of the Box-Muller arithmetic and summed behind it where state,
// proposal, normals and six rows fit the register budget without costing a wave of occupancy; above that only the first pair
// is, and the others are gathered and added pair by pair behind the normals
#ifndef DEMCZ_CR_INFLIGHT_MAX_D
#define DEMCZ_CR_INFLIGHT_MAX_D 10
#endif

// ADAPT: the kernel has a third argument, CrossoverAdaptParams -- AP is that one type, and empty otherwise, so that the kernel
// without adaptation keeps the two kernel arguments it has
template <int TARGET, int D, bool ADAPT = false, class... AP>
__global__ void __launch_bounds__(WINDOW_BS) window_kernel_cr(const WindowParams P, const CrossoverParams C, const AP... adapt_args)
{
    static_assert(D >= 1 && D <= 64, "the subset is a 64-bit mask");
    static_assert(sizeof...(AP) == (ADAPT ? 1 : 0), "window_kernel_cr<TARGET, D> or window_kernel_cr<TARGET, D, true, CrossoverAdaptParams>");
    const int64_t c = (int64_t)blockIdx.x * WINDOW_BS + threadIdx.x;
    if (c >= P.N) return;
    [[maybe_unused]] CrossoverParams Cl;      // ADAPT: C with the cumulative weights as device memory holds them now
    [[maybe_unused]] CrDist cd;
    [[maybe_unused]] double rsdc[ADAPT ? D : 1];      // the spread, launch-invariant: in scalar registers like the target's constants
    if constexpr (ADAPT) {
        const CrossoverAdaptParams& A = cr_adapt_params(adapt_args...);
        Cl = cr_adapted(C, A);
        cd.clear();
#pragma unroll
        for (int p = 0; p < D; ++p) rsdc[p] = uniform_double(A.rsd[p]);
    }

    double x[D];
#pragma unroll
    for (int p = 0; p < D; ++p) x[p] = P.Xcur[c + P.N * p];
    double lp = P.lpcur[c];
    // target constants in scalar registers where window_kernel keeps them there
    constexpr bool LOCAL_TARGET = (TARGET == TARGET_MVNORMAL && D <= 10) || TARGET == TARGET_ISO_QUAD;
    [[maybe_unused]] double muc[LOCAL_TARGET ? D : 1], Wc[(LOCAL_TARGET && TARGET == TARGET_MVNORMAL) ? D * (D + 1) / 2 : 1], epsc[LOCAL_TARGET ? D : 1];
    if constexpr (LOCAL_TARGET) {
#pragma unroll
        for (int p = 0; p < D; ++p) { muc[p] = uniform_double(P.tp.mu[p]); epsc[p] = uniform_double(P.eps[p]); }
        if constexpr (TARGET == TARGET_MVNORMAL) {
#pragma unroll
            for (int i = 0; i < D * (D + 1) / 2; ++i) Wc[i] = uniform_double(P.tp.Wp[i]);
        }
    }
    [[maybe_unused]] const double c0c = P.tp.c0;
    // the log-density of a point: the operation sequence of target_logp (one block: never grouped)
    auto logp_of = [&](const double (&xq)[D]) -> double {
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
    int to_b = P.to_boundary;            // countdown to the next K boundary
    int64_t nb = 0;                      // boundaries passed inside this launch
    unsigned int cnt_total = 0, cnt_first = 0;
    const unsigned long long speak64 = __builtin_amdgcn_ballot_w64(true);      // every lane still here runs a chain
    CrCounts cc;
    cc.clear();
    const int ncr = C.ncr, delta_max = C.delta_max;
    constexpr bool INFLIGHT = D <= DEMCZ_CR_INFLIGHT_MAX_D;
    constexpr int NHELD = INFLIGHT ? CR_MAX_PAIRS : 1;      // pairs whose rows are held across the normals

    for (int gi = 0; gi < P.ngen; ++gi) {
        const double lp_gen0 = lp;
        uint64_t r1, r2;
        rng_next(st, r1, r2);
        int m, delta, pstar;
        if constexpr (ADAPT) cr_choices(Cl, r1, r2, D, m, delta, pstar);
        else cr_choices(C, r1, r2, D, m, delta, pstar);
        // the pairs: every block is drawn (the positions are fixed), the rows of pair j only where j <= delta
        uint64_t i1[CR_MAX_PAIRS], i2[CR_MAX_PAIRS];
        double za[NHELD][D], zb[NHELD][D];
#pragma unroll
        for (int j = 0; j < CR_MAX_PAIRS; ++j) {
            i1[j] = i2[j] = 0;
            if (j < delta_max) {                 // wave-uniform
                rng_next(st, r1, r2);
                draw_rows(r1, r2, (uint64_t)P.M, i1[j], i2[j]);
            }
            if (j < NHELD) {
#pragma unroll
                for (int p = 0; p < D; ++p) za[j][p] = zb[j][p] = 0.0;
                if (j == 0 || j < delta) {       // (delta >= 1)
                    load_row<D>(P.Z + (int64_t)i1[j] * P.ZS, za[j]);
                    load_row<D>(P.Z + (int64_t)i2[j] * P.ZS, zb[j]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the subset
        unsigned long long mask = 0ull;
#pragma unroll
        for (int q = 0; q < (D + 3) / 4; ++q) {
            rng_next(st, r1, r2);
            const uint32_t w[4] = {(uint32_t)r1, (uint32_t)(r1 >> 32), (uint32_t)r2, (uint32_t)(r2 >> 32)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (4 * q + t < D) mask |= cr_selects(w[t], ncr, m) ? (1ull << (4 * q + t)) : 0ull;
            }
        }
        mask = (mask == 0ull) ? (1ull << pstar) : mask;
        const int dsel = __builtin_popcountll(mask);
        // the normals
        double zn[((D + 1) / 2) * 2];
#pragma unroll
        for (int pr = 0; pr < (D + 1) / 2; ++pr) {
            rng_next(st, r1, r2);
            normal_pair(r1, r2, zn[2 * pr], zn[2 * pr + 1]);
        }
        rng_next(st, r1, r2);
        const double logu = dm_log(u_open(r1));
        // the difference sum
        double s[D];
#pragma unroll
        for (int p = 0; p < D; ++p) s[p] = za[0][p] - zb[0][p];
#pragma unroll
        for (int j = 1; j < CR_MAX_PAIRS; ++j) {
            if constexpr (INFLIGHT) {
#pragma unroll
                for (int p = 0; p < D; ++p) {
                    const double dj = za[j][p] - zb[j][p];
                    const double sj = s[p] + dj;
                    s[p] = (j < delta) ? sj : s[p];
                }
            } else {
                if (j < delta) {
                    double ra[D], rb[D];
                    load_row<D>(P.Z + (int64_t)i1[j] * P.ZS, ra);
                    load_row<D>(P.Z + (int64_t)i2[j] * P.ZS, rb);
#pragma unroll
                    for (int p = 0; p < D; ++p) {
                        const double dj = ra[p] - rb[p];
                        s[p] = s[p] + dj;
                    }
                }
            }
        }
        const double scale = P.gamma / sqrt((double)(2 * delta * dsel));
        double xp[D];
#pragma unroll
        for (int p = 0; p < D; ++p) {
            const double t1 = scale * s[p];
            const double t2 = (LOCAL_TARGET ? epsc[p] : P.eps[p]) * zn[p];
            const double dlt_p = t1 + t2;
            const double moved = x[p] + dlt_p;
            xp[p] = ((mask >> p) & 1ull) ? moved : x[p];
        }
        const double lpp = logp_of(xp);
        double dlt = lpp - lp;
        if (P.temperature) dlt = dlt / P.temperature[gi];
        const bool acc = logu < dlt;
        if constexpr (ADAPT) {
            const CrossoverAdaptParams& A = cr_adapt_params(adapt_args...);
            if (A.accumulate) {                 // launch-uniform
                double J = 0.0;
#pragma unroll
                for (int p = 0; p < D; ++p) {
                    const double df = xp[p] - x[p];
                    const double tp = df * rsdc[p];
                    const double t2 = tp * tp;
                    J = J + t2;
                }
                cd.add(m, acc ? cr_quantise(J) : 0ull);
            }
        }
#pragma unroll
        for (int p = 0; p < D; ++p) x[p] = acc ? xp[p] : x[p];
        lp = acc ? lpp : lp;
        cc.count(ncr, m, acc, speak64);
        {
            const unsigned int k = wave_count_changed(lp, lp_gen0, speak64);
            cnt_total += k;
            cnt_first = (gi == 0) ? k : cnt_first;
        }
        const int64_t slot = P.slot_first + gi;
        if (P.chain) {
#pragma unroll
            for (int p = 0; p < D; ++p) P.chain[c + P.N * (p + (int64_t)D * slot)] = x[p];
            P.logobj[c + P.N * slot] = lp;
        }
        if (--to_b == 0) {                  // generation divisible by K: the append of any generation
            to_b = P.K;
            if (P.do_append) store_row<D>(P.Zw + (P.M_append + nb * P.N + c) * P.ZS, x);
            if (P.snap) {
#pragma unroll
                for (int p = 0; p < D; ++p) P.snap[nb * P.N * D + c + P.N * p] = x[p];
            }
            ++nb;
        }
    }
#pragma unroll
    for (int p = 0; p < D; ++p) P.Xcur[c + P.N * p] = x[p];
    P.lpcur[c] = lp;
    wave_store_counts(P, blockIdx.x, cnt_total, cnt_first);
    cc.add_to(C.counts);
    if constexpr (ADAPT) {
        const CrossoverAdaptParams& A = cr_adapt_params(adapt_args...);
        if (A.accumulate) cd.add_to(A.slots, cc.tried, __builtin_popcountll(speak64));
    }
}

// run-time d: x and the proposal in LDS (2 d columns of WINDOW_BS doubles, dynamic), the rows read where they are used; the
// normals are consumed pair by pair as they are made, so they need no column of their own
template <int TARGET, bool ADAPT = false, class... AP>
__global__ void __launch_bounds__(WINDOW_BS) window_kernel_cr_generic(const WindowParams P, const CrossoverParams C, const AP... adapt_args)
{
    static_assert(sizeof...(AP) == (ADAPT ? 1 : 0), "window_kernel_cr_generic<TARGET> or window_kernel_cr_generic<TARGET, true, CrossoverAdaptParams>");
    extern __shared__ double lds[];
    const int d = P.d;
    double* xs = lds;                         // d x BS
    double* xps = lds + d * WINDOW_BS;        // d x BS
    const int64_t c = (int64_t)blockIdx.x * WINDOW_BS + threadIdx.x;
    if (c >= P.N) return;
    const int tid = threadIdx.x;
    [[maybe_unused]] CrossoverParams Cl;
    [[maybe_unused]] CrDist cd;
    if constexpr (ADAPT) {
        Cl = cr_adapted(C, cr_adapt_params(adapt_args...));
        cd.clear();
    }

    for (int p = 0; p < d; ++p) xs[p * WINDOW_BS + tid] = P.Xcur[c + P.N * p];
    double lp = P.lpcur[c];
    rng_state st;
    rng_seek(st, P.seed, (uint64_t)(P.chain_id0 + c), (uint64_t)(P.g_first - 1) * (uint64_t)P.S);
    int to_b = P.to_boundary;
    int64_t nb = 0;
    unsigned int cnt_total = 0, cnt_first = 0;
    const unsigned long long speak64 = __builtin_amdgcn_ballot_w64(true);
    CrCounts cc;
    cc.clear();
    const int ncr = C.ncr, delta_max = C.delta_max;

    for (int gi = 0; gi < P.ngen; ++gi) {
        const double lp_gen0 = lp;
        uint64_t r1, r2;
        rng_next(st, r1, r2);
        int m, delta, pstar;
        if constexpr (ADAPT) cr_choices(Cl, r1, r2, d, m, delta, pstar);
        else cr_choices(C, r1, r2, d, m, delta, pstar);
        const double* ra[CR_MAX_PAIRS];
        const double* rb[CR_MAX_PAIRS];
#pragma unroll
        for (int j = 0; j < CR_MAX_PAIRS; ++j) {
            uint64_t i1 = 0, i2 = 0;
            if (j < delta_max) {
                rng_next(st, r1, r2);
                draw_rows(r1, r2, (uint64_t)P.M, i1, i2);
            }
            ra[j] = P.Z + (int64_t)i1 * P.ZS;
            rb[j] = P.Z + (int64_t)i2 * P.ZS;
        }
        unsigned long long mask = 0ull;
        for (int q = 0; q < (d + 3) / 4; ++q) {
            rng_next(st, r1, r2);
            const uint32_t w[4] = {(uint32_t)r1, (uint32_t)(r1 >> 32), (uint32_t)r2, (uint32_t)(r2 >> 32)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int p = 4 * q + t;
                if (p < d && cr_selects(w[t], ncr, m)) mask |= 1ull << p;
            }
        }
        mask = (mask == 0ull) ? (1ull << pstar) : mask;
        const int dsel = __builtin_popcountll(mask);
        const double scale = P.gamma / sqrt((double)(2 * delta * dsel));
        for (int pr = 0; pr < (d + 1) / 2; ++pr) {
            rng_next(st, r1, r2);
            double z01[2];
            normal_pair(r1, r2, z01[0], z01[1]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int p = 2 * pr + t;
                if (p < d) {
                    double xv = xs[p * WINDOW_BS + tid];
                    if ((mask >> p) & 1ull) {
                        double sp = ra[0][p] - rb[0][p];
#pragma unroll
                        for (int j = 1; j < CR_MAX_PAIRS; ++j) {
                            if (j < delta) {
                                const double dj = ra[j][p] - rb[j][p];
                                sp = sp + dj;
                            }
                        }
                        const double t1 = scale * sp;
                        const double t2 = P.eps[p] * z01[t];
                        const double dlt_p = t1 + t2;
                        xv = xv + dlt_p;
                    }
                    xps[p * WINDOW_BS + tid] = xv;
                }
            }
        }
        rng_next(st, r1, r2);
        const double logu = dm_log(u_open(r1));
        const double lpp = target_logp<TARGET, 0>(P.tp, d, [&](int j) { return xps[j * WINDOW_BS + tid]; });
        double dlt = lpp - lp;
        if (P.temperature) dlt = dlt / P.temperature[gi];
        const bool acc = logu < dlt;
        if constexpr (ADAPT) {
            const CrossoverAdaptParams& A = cr_adapt_params(adapt_args...);
            if (A.accumulate) {                 // launch-uniform
                double J = 0.0;
                for (int p = 0; p < d; ++p) {
                    const double df = xps[p * WINDOW_BS + tid] - xs[p * WINDOW_BS + tid];
                    const double tp = df * A.rsd[p];
                    const double t2 = tp * tp;
                    J = J + t2;
                }
                cd.add(m, acc ? cr_quantise(J) : 0ull);
            }
        }
        if (acc) {
            for (int p = 0; p < d; ++p) xs[p * WINDOW_BS + tid] = xps[p * WINDOW_BS + tid];
            lp = lpp;
        }
        cc.count(ncr, m, acc, speak64);
        {
            const unsigned int k = wave_count_changed(lp, lp_gen0, speak64);
            cnt_total += k;
            cnt_first = (gi == 0) ? k : cnt_first;
        }
        const int64_t slot = P.slot_first + gi;
        if (P.chain) {
            for (int p = 0; p < d; ++p) P.chain[c + P.N * (p + (int64_t)d * slot)] = xs[p * WINDOW_BS + tid];
            P.logobj[c + P.N * slot] = lp;
        }
        if (--to_b == 0) {
            to_b = P.K;
            for (int p = 0; p < d; ++p) {
                const double xv = xs[p * WINDOW_BS + tid];
                if (P.do_append) P.Zw[(P.M_append + nb * P.N + c) * P.ZS + p] = xv;
                if (P.snap) P.snap[nb * P.N * d + c + P.N * p] = xv;
            }
            ++nb;
        }
    }
    for (int p = 0; p < d; ++p) P.Xcur[c + P.N * p] = xs[p * WINDOW_BS + tid];
    P.lpcur[c] = lp;
    wave_store_counts(P, blockIdx.x, cnt_total, cnt_first);
    cc.add_to(C.counts);
    if constexpr (ADAPT) {
        const CrossoverAdaptParams& A = cr_adapt_params(adapt_args...);
        if (A.accumulate) cd.add_to(A.slots, cc.tried, __builtin_popcountll(speak64));
    }
}

#ifndef DEMCZ_PROGRAM_TARGET
// ---- the update of the adapted weights ("adaptation of the class weights") ---------------------------------------
struct CrAdaptUpdate {
    const double* X;                       // the chains as they stand, X[c + N p]
    int64_t N;
    int32_t d, ncr, min_weight, nwg;       // nwg: workgroups of a window launch (slots)
    int32_t* weights;                      // [8]
    uint32_t* cum;                         // [8]: what the next launch reads
    long long* updates;
    double* rsd;                           // [d]
    unsigned long long* slots;             // [nwg][8][2]
};

// the sum of v over the chains of one column, in THE order of the specification: lane l adds its chains c = l, l + 64, ... in
// increasing c onto 0.0, then a_l = a_l + a_(l + s) for s = 32 ... 1; every lane returns lane 0's sum
template <class F>
__device__ __forceinline__ double cr_column_sum(int64_t N, F&& v)
{
    double a = 0.0;
    for (int64_t c = threadIdx.x; c < N; c += 64) a = a + v(c);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) a = a + __shfl_down(a, s, 64);
    return __shfl(a, 0, 64);
}

// grid d + 1 (an update) or d (the start of adaptation: the spread only), 64 lanes.  Block p < d: rsd_p.  Block d: the slots' sums,
// the weight rule in one lane, and the totals back into workgroup 0's slots with the others zeroed.
template <int LANES>
__global__ void __launch_bounds__(LANES) cr_adapt_kernel(const CrAdaptUpdate U)
{
    static_assert(LANES == 64, "one wave");
    const int lane = (int)threadIdx.x;
    if ((int)blockIdx.x < U.d) {
        const double* col = U.X + U.N * (int64_t)blockIdx.x;
        const double sum = cr_column_sum(U.N, [&](int64_t c) { return col[c]; });
        const double mean = sum / (double)U.N;
        const double ss = cr_column_sum(U.N, [&](int64_t c) { const double t = col[c] - mean; return t * t; });
        const double var = ss / (double)(U.N - 1);
        const double r = 1.0 / sqrt(var);
        if (lane == 0) U.rsd[blockIdx.x] = (var > 0.0 && var < __builtin_inf()) ? r : 0.0;
        return;
    }
    unsigned long long tot = 0ull;
    if (lane < 2 * CR_MAX_CLASSES) {
        for (int w = 0; w < U.nwg; ++w) tot += U.slots[(size_t)w * (2 * CR_MAX_CLASSES) + lane];
        U.slots[lane] = tot;
        for (int w = 1; w < U.nwg; ++w) U.slots[(size_t)w * (2 * CR_MAX_CLASSES) + lane] = 0ull;
    }
    double r[CR_MAX_CLASSES];
    double R = 0.0;
#pragma unroll
    for (int k = 0; k < CR_MAX_CLASSES; ++k) {
        const unsigned long long dist = __shfl(tot, 2 * k, 64), tried = __shfl(tot, 2 * k + 1, 64);
        r[k] = (k < U.ncr && tried > 0ull) ? (double)dist / (double)tried : 0.0;
        if (k < U.ncr) R = R + r[k];
    }
    if (lane != 0) return;
    if (R > 0.0) {
        uint32_t sum = 0u;
#pragma unroll
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            if (k < U.ncr) {
                const double share = r[k] / R;
                const double sc = share * 65536.0;
                const int32_t w = (int32_t)sc;
                const int32_t wk = w > U.min_weight ? w : U.min_weight;
                U.weights[k] = wk;
                sum += (uint32_t)wk;
            }
            U.cum[k] = sum;
        }
    }
    *U.updates = *U.updates + 1;
}

// the built-in instantiations live in demcz_crossover_inst.hip; this hands out their host symbols.  *dyn_lds: dynamic LDS bytes of
// the launch (the run-time-d form).  nullptr: no built-in kernel for that target (program targets bring their own).
// adapt: the ADAPT twin, which lives with cr_adapt_kernel in demcz_crossover_adapt_inst.hip (a unit of its own: the build is
// parallel over units).
const void* crossover_kernel_fn(int target_kind, int d, size_t* dyn_lds, bool adapt = false);
const void* crossover_adapt_kernel_fn(int target_kind, int d, size_t* dyn_lds);
const void* crossover_adapt_update_fn();
#endif

}  // namespace demcz
