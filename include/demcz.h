/*
 * demcz.h -- C ABI of libdemcz_hip.so, the MI355X (gfx950) DEMCz chain-update engine.
 *
 * The reference (chrished/DEMC.jl) is a pure-Julia package with no FFI of its own; the seam this
 * ABI occupies is the call the drivers make into runchain!:
 *     src/demcz.jl:30-33         for ig = 1:Ngeneration, for ic = 1:N  runchain!(ic, ig, ig, ...)
 *     src/demcz_anneal.jl:39-42  same loop, tempered
 * Everything below that call (runchain! :80-93, update_blocks :167-172,
 * update_demcz_chain_block :174-195, accept :197-203, and the annealer's overloads
 * demcz_anneal.jl:67-80,142-178) runs on the device; the autostop statistic
 * (Rhat_gelman, src/utils.jl:2-20, called at demcz.jl:41) and the acceptance counts
 * (demcz.jl:42, demcz_anneal.jl:50) are device reductions over the on-device history.
 * The Julia-side binding a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns an int32 status (0 = OK);
 *     no exceptions or longjmp cross the boundary; demcz_last_error() gives the message.
 *   - All matrices are COLUMN-MAJOR exactly as Julia lays them out (DEMC.jl:10-15), so a
 *     Matrix{Float64} / Array{Float64,3} is passed by pointer without transposition:
 *       X, Xcurrent   N x d        element (ic, ip)      at ic + N*ip
 *       Z             M x d        element (row, ip)     at row + ldZ*ip   ("parameter-major")
 *       chain         N x d x G    element (ic, ip, ig)  at ic + N*(ip + d*ig)
 *       log_obj       N x G        element (ic, ig)      at ic + N*ig
 *   - Indices are 0-based on this side; generations are 1-based like the reference's `ig`
 *     because `ig % K == 0` (demcz.jl:88) and the temperature schedule depend on the value.
 *   - Host pointers unless a name ends in `_device`.  The caller owns every host buffer; the
 *     library owns device memory.
 *   - A handle is bound to one device and one stream and is not thread-safe.
 *   - Work is enqueued asynchronously on the handle's stream; functions that return data to
 *     host memory synchronise that stream first.
 */
#ifndef DEMCZ_H
#define DEMCZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct demcz_handle demcz_handle;

enum demcz_status {
    DEMCZ_OK = 0,
    DEMCZ_ERR_INVALID_ARGUMENT = 1,
    DEMCZ_ERR_HIP = 2,            /* a HIP runtime call failed (message has hipGetErrorString) */
    DEMCZ_ERR_CAPACITY = 3,       /* Z row capacity or history capacity exceeded               */
    DEMCZ_ERR_STATE = 4,          /* call order: e.g. run before set_state                      */
    DEMCZ_ERR_NO_DEVICE = 5,      /* no gfx950 device visible: there is NO CPU fallback         */
    DEMCZ_ERR_COMM = 6            /* sharded run: an RCCL call failed, RCCL reported an asynchronous error, or a wait on the
                                     exchange made no progress within the deadline (demcz_set_comm_timeout) -- a peer rank is
                                     dead or stalled.  Both communicators have been aborted; the handle only accepts
                                     demcz_destroy / demcz_last_error from now on.  Restart the job in fresh processes.  */
};

/* User log-densities the device can evaluate (the reference takes an arbitrary Julia closure,
 * demcz.jl:189; the BASELINE configs use these three -- SURVEY.md 8(a) a11). */
enum demcz_target_kind {
    DEMCZ_TARGET_MVNORMAL = 0,    /* logpdf(MvNormal(mu, Sigma), x)   test/example_normpdf.jl:13-16 */
    DEMCZ_TARGET_ISO_QUAD = 1,    /* -sum((x - mu).^2)                test/test_anneal.jl:10        */
    DEMCZ_TARGET_LINREG_SSE = 2,  /* -0.5*sum((y - X*b).^2)           test/example_linreg.jl:32     */
    DEMCZ_TARGET_HOST_CALLBACK = 3, /* arbitrary closure on the host: demcz_propose/accept_commit   */
    DEMCZ_TARGET_PROGRAM = 4      /* a log-density written as HIP C++, compiled at run time: demcz_set_program */
};

/* Mirrors the fields of DEMCopt the hot path reads (src/DEMC.jl:24-39: N, K, Nblocks,
 * blockindex, eps_scale) plus what a device engine needs.  POD; copied by demcz_create. */
typedef struct demcz_config {
    int64_t N;                    /* chains on THIS handle (DEMCopt.N, or the local shard of it)   */
    int64_t chain_id0;            /* global id of local chain 0 (0 when not sharded): the chain's
                                     RNG stream is Philox subsequence chain_id0 + ic, so results do
                                     not depend on how chains are sharded over GPUs                */
    int32_t d;                    /* Npar                                                           */
    int32_t K;                    /* DEMCopt.K: every K-th generation the current states join Z     */
    int64_t Mcap;                 /* row capacity of Z: M0 + ceil(N_total*Ngeneration/K), demcz.jl:11 */
    int64_t Gcap;                 /* generations of chain/log_obj history kept on the device        */
    int32_t Nblocks;              /* DEMCopt.Nblocks                                                */
    const int32_t* block_offsets; /* CSR over DEMCopt.blockindex: Nblocks+1 offsets ...             */
    const int32_t* block_indices; /* ... into 0-based parameter indices                             */
    const double* eps_scale;      /* DEMCopt.eps_scale, d values                                    */
    uint64_t seed;                /* Philox4x32-10 key (rocRAND-compatible stream layout)           */
    int32_t device_id;            /* HIP device ordinal                                             */
    int32_t target_kind;          /* enum demcz_target_kind                                         */
    const double* mu;             /* MVNORMAL / ISO_QUAD: d                                         */
    const double* W;              /* MVNORMAL: d x d column-major lower-triangular inv(chol(Sigma)) */
    double c0;                    /* MVNORMAL: -0.5*(d*log(2pi) + logdet(Sigma))                    */
    const double* design;         /* LINREG_SSE: nobs x d column-major                              */
    const double* yobs;           /* LINREG_SSE: nobs                                               */
    int64_t nobs;
    void* stream;                 /* hipStream_t to enqueue on, or NULL: the library makes its own  */
    int32_t lanes_per_chain;      /* kernel layout: 0 = let the library choose; 1 = one lane per chain,
                                     fused (throughput layout, large N); 8 / 16 = that many lanes
                                     cooperate on a chain; DEMCZ_LAYOUT_SPLIT = producer workgroups
                                     make the state-independent draws one launch ahead, consumer
                                     lanes run the chains, and on one GPU a launch runs through many
                                     K boundaries (small N); DEMCZ_LAYOUT_SPLIT_WAVE = the same with
                                     one wavefront per chain that resolves five generations per pass
                                     (smallest N; MvNormal at every d in 2..32, the isotropic quadratic
                                     at d in 6..32).  The regression target: d = 10 on the FP64 matrix
                                     instruction (split layouts), any other d in 2..28 on sixteen
                                     lanes per chain with helper waves.  Results are bit-identical.
                                     DEMCZ_LAYOUT_PROGRAM_WAVE: a program target on the wave-per-chain
                                     layout (see "Program targets" below; only with
                                     DEMCZ_TARGET_PROGRAM, which otherwise takes 0 or 1). */
    int32_t reserved0;
} demcz_config;

#define DEMCZ_LAYOUT_SPLIT 100
#define DEMCZ_LAYOUT_SPLIT_WAVE 164
#define DEMCZ_LAYOUT_PROGRAM_WAVE 264

/* Program targets (DEMCZ_TARGET_PROGRAM): the closure of demcz.jl:189 as a small HIP C++ function the library compiles for
 * gfx950 at run time (hipRTC) together with its one-lane window kernel, so that it runs on the device like a built-in target
 * (same Philox streams, draw order, history, archive, R-hat check and annealing; one launch per K-window).  The source defines
 *     __device__ double demcz_logobj(const double* x, const double* data, int64_t ndata);
 * x: the DEMCZ_D (= d, a macro the program may use) values of the proposal; data: the ndata doubles given to demcz_set_program
 * (device memory, read-only).  Compiled with --offload-arch=gfx950 -O3 -ffp-contract=off followed by `options` (space-separated,
 * e.g. "-DNOBS=1000"; may be NULL): with contraction off a fused multiply-add happens only where fma() is written, so what the
 * source says is what is computed, bit for bit.  Handles of a program target take lanes_per_chain 0 or 1 (both: one lane per
 * chain) or DEMCZ_LAYOUT_PROGRAM_WAVE (below) and 1 <= d <= 32; the target fields of demcz_config are not read.
 *   demcz_program_check  compiles the program for dimension d and needs no device.  DEMCZ_OK, or DEMCZ_ERR_INVALID_ARGUMENT with
 *                        the compiler log (user's line numbers, file "program") in demcz_last_error(NULL).
 *   demcz_set_program    compiles the program (or takes it from the process-wide cache: a second handle with the same program and
 *                        options does not recompile), loads it on the handle's device and copies data (ndata >= 0 doubles, NULL
 *                        when 0) to device memory the handle owns.  Once per handle, before the first demcz_set_state; until it
 *                        has succeeded demcz_set_state and the calls that evaluate the target return DEMCZ_ERR_STATE.  A compile
 *                        error is DEMCZ_ERR_INVALID_ARGUMENT with the log in demcz_last_error(h); the handle stays usable for a
 *                        corrected demcz_set_program. */
int32_t demcz_program_check(int32_t d, const char* source, const char* options);
/* Program targets on the wave-per-chain layout (opt-in: lanes_per_chain = DEMCZ_LAYOUT_PROGRAM_WAVE at demcz_create).  The same
 * source, contract and bits as above, compiled into the split layout's wave-per-chain consumer instead of the one-lane kernel: one
 * wavefront per chain resolves up to five generations a pass, lane n of it evaluating demcz_logobj on candidate n of the 31 nodes
 * of the pass's accept / reject tree; the draws come from the library's producer kernel, and on one GPU a launch runs through
 * many K boundaries with the rows handed over inside it (one launch per K-window where N is more than such a launch holds).
 * Measured at N = 1024 (where a launch of it holds every chain): 4.6 to 11.7 times less kernel time per K-window than the
 * one-lane kernel, which stays the default and the only one for N > 2048.  Valid only with DEMCZ_TARGET_PROGRAM, one block 0..d-1 in order, 2 <= d <= 32, N <= 2048 and an archive
 * reachable by 32-bit offsets (Mcap * 8 * (d rounded up to a multiple of 8) < 2^32); anything else is
 * DEMCZ_ERR_INVALID_ARGUMENT at demcz_create with a message that names the condition.  demcz_comm_init and demcz_peer_group
 * return DEMCZ_ERR_STATE on such a handle (host-driven sharding -- demcz_set_external_append, demcz_append_rows -- works).
 * What the layout asks of demcz_logobj beyond the contract above: it is called for ALL 31 candidates of a pass, most of which the
 * chain never takes (candidates several accepted steps away from the current state among them), so it must be a pure function of
 * (x, data) -- no state kept between calls, no writes to data -- that terminates for every finite x.  A NaN result rejects, as
 * on the one-lane layout.  INFINITY and NAN are defined for the program as <math.h> defines them (return -INFINITY outside a
 * bounded support).
 *   demcz_program_check_layout  demcz_program_check for the unit a handle with this lanes_per_chain would compile (0, 1 or
 *                        DEMCZ_LAYOUT_PROGRAM_WAVE; the latter needs 2 <= d <= 32): a compiler error of the wave unit -- registers,
 *                        a construct that does not inline -- shows without a device.  Fills the same process-wide cache. */
int32_t demcz_program_check_layout(int32_t d, const char* source, const char* options, int32_t lanes_per_chain);
int32_t demcz_set_program(demcz_handle* h, const char* source, const char* options, const double* data, int64_t ndata);

/* Version of this header's ABI; demcz_abi_version() must return the same number. */
#define DEMCZ_ABI_VERSION 1
int32_t demcz_abi_version(void);

/* Create / destroy.  Replaces the driver's setup, demcz.jl:10-12 and :24 (allocation of the
 * padded Z, M, and the MC history arrays) -- here as device buffers sized from cfg. */
int32_t demcz_create(demcz_handle** out, const demcz_config* cfg);
int32_t demcz_destroy(demcz_handle* h);
const char* demcz_last_error(const demcz_handle* h);   /* h may be NULL: last create error */

/* Upload the start state: demcz.jl:13-22.  X is N x d (ld N); logp is N values or NULL to have
 * the device evaluate the target at X (demcz.jl:17); Z is M0 x d with leading dimension ldZ;
 * 2 <= M0 <= Mcap (two distinct archive rows are needed, demcz.jl:176-179).
 * Non-finite values are accepted, in X, logp and Z alike (+-Inf, NaN, -0.0, subnormals), as the reference accepts them: +-Inf and
 * NaN log-densities follow the accept rule (log u < lp' - lp, strict: a NaN difference rejects) and the changed rule
 * ((lp_after - lp_before) != 0: a NaN difference counts) bit for bit in every layout; signs of zero and subnormals are kept; which
 * NaN (sign, payload) comes out of an operation is unspecified.  One bit pattern is reserved and must not occur in X or Z:
 * 0xFFF4DEADC0DE5EED, the sentinel the unwritten part of the archive holds. */
int32_t demcz_set_state(demcz_handle* h, const double* X, const double* logp,
                        const double* Z, int64_t ldZ, int64_t M0);

/* Download the current state: mc.Xcurrent, mc.log_objcurrent (DEMC.jl:13-14), Z[1:M,:] and M
 * (demcz.jl:51).  Any pointer may be NULL.  Z is written with leading dimension ldZ >= M. */
int32_t demcz_get_state(demcz_handle* h, double* X, double* logp, double* Z, int64_t ldZ, int64_t* M);

/* Z[1:M,:] (demcz.jl:51) in a pinned host buffer of the library's pool, M x d column-major with leading dimension M: no page
 * faults of a fresh array under the copy (41 MB at the end of a C2 run).  The caller gives *Z back with demcz_release_host_buffer. */
int32_t demcz_get_archive_pinned(demcz_handle* h, double** Z, int64_t* M);

/* Map generation index -> history slot: generation g is stored at slot g - g0 - 1, so the
 * device keeps generations g0+1 .. g0+Gcap.  Default g0 = 0. */
int32_t demcz_set_history_origin(demcz_handle* h, int64_t g0);

/* Run generations g_from..g_to (inclusive, 1-based) for all N chains: the loop demcz.jl:30-33 /
 * demcz_anneal.jl:39-42 with runchain! and everything below it.  gamma is DEMCopt.gamma (a
 * per-call scalar so the annealer's adaptation, demcz_anneal.jl:48-57, can change it between
 * calls).  temperature is NULL for the sampler or g_to-g_from+1 host values (one per
 * generation, temperaturefun(ig, ...) of demcz_anneal.jl:69) for the tempered accept.
 * Asynchronous.  Chains are updated synchronously within a generation (all proposals of a
 * generation see the same M; the N rows are appended after it -- SURVEY.md Q2).
 * When the handle is one shard of a multi-GPU run (demcz_comm_init was called) the K-boundary
 * append all-gathers the shards' rows over RCCL so every replica of Z stays identical. */
int32_t demcz_run(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature);

int32_t demcz_synchronize(demcz_handle* h);

/* Copy history out: mc.chain[:, :, g_from:g_to] and mc.log_obj[:, g_from:g_to] (DEMC.jl:11-12).
 * Either pointer may be NULL. */
int32_t demcz_get_history(demcz_handle* h, int64_t g_from, int64_t g_to, double* chain, double* log_obj);

/* Streamed history.  mc.chain / mc.log_obj of a C2 run are half a gigabyte that only exists to be handed back (DEMC.jl:10-12);
 * copied after the run they cost four times what the run does.  With streaming enabled (before demcz_run) the library keeps
 * pinned host mirrors of both arrays -- same layout, generation g at slot g - g0 - 1 -- and every demcz_run call's generations
 * leave on a copy stream while the compute stream goes on with the next call.
 *   demcz_get_history_view   waits for the copies of g_from..g_to (redoing a voided LIVE slab first) and returns pointers INTO the
 *                            mirrors: N x d x G and N x G column-major, no further copy.  Valid until the handle is destroyed ...
 *   demcz_detach_history     ... unless the mirrors are detached: they then belong to the caller (a Julia Array made with
 *                            unsafe_wrap, a NumPy array over the pointer) until demcz_release_host_buffer gives each back.
 * The mirrors come from a process-wide pool of pinned buffers: a second run of the same shape allocates nothing. */
int32_t demcz_history_stream(demcz_handle* h, int32_t enabled);
int32_t demcz_get_history_view(demcz_handle* h, int64_t g_from, int64_t g_to, double** chain, double** log_obj);
int32_t demcz_detach_history(demcz_handle* h, void** chain_base, void** logobj_base);
int32_t demcz_release_host_buffer(void* base);

/* The library keeps the big buffers of destroyed handles (device: history + archive, at most 6 GiB; pinned host: history mirrors,
 * at most 3 GiB) for the next handle of the process.  demcz_pool_trim gives everything cached back to the runtime (it is also
 * what the library does by itself when one of its own allocations fails); either pointer may be NULL. */
int32_t demcz_pool_trim(int64_t* device_bytes_freed, int64_t* pinned_bytes_freed);

/* changed[g - g_from] = number of local chains whose log_obj at generation g differs from the
 * one before it -- the event counted by sum(diff(log_obj, dims=2) .!= 0) at demcz.jl:42 and
 * demcz_anneal.jl:50. */
int32_t demcz_get_changed(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t* changed);

/* *total = sum over g in g_from..g_to of the changed[] counts above -- the acceptance count of the annealer's gamma
 * adaptation (demcz_anneal.jl:50) and of the autostop warning (demcz.jl:42).  The window kernels count it as they
 * go: one wavefront ballot of "this chain's log_obj changed" per generation, popcount into a scalar register, two
 * words per wave per launch (no atomics, no second pass over log_obj); when g_from..g_to is covered by whole
 * launches (it is, for the drivers' windows) the answer is the sum of those words and *from_ballots = 1; otherwise
 * it is counted from the history like demcz_get_changed (*from_ballots = 0).  from_ballots may be NULL.
 * Works on handles without a history window (Gcap = 0) in the first case. */
int32_t demcz_get_changed_total(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t* total, int32_t* from_ballots);

/* Split-chain Gelman-Rubin statistic over generations g_from..g_to of the on-device history:
 * Rhat_gelman(chain[:, :, g_from:g_to], N, g_to-g_from+1, d), src/utils.jl:2-20, as called by
 * the autostop at demcz.jl:41.  rhat receives d values.  On a sharded handle the partial
 * moments are all-reduced so every rank gets the statistic over all N_total chains. */
int32_t demcz_rhat(demcz_handle* h, int64_t g_from, int64_t g_to, double* rhat);

/* The two reduction stages of demcz_rhat over the LOCAL chains only, for hosts that reduce
 * across shards themselves: stage 0 -> out[0..d) = sum_j mean_j over the 2N local split-chains;
 * stage 1 (grand = the global mean per parameter, d values) -> out[0..d) = sum_j (mean_j -
 * grand)^2, out[d..2d) = sum_j s_j^2.  The caller sums `out` over shards between the stages
 * and finishes with utils.jl:13-18. */
int32_t demcz_rhat_partial(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t stage,
                           const double* grand, double* out);

/* Effective sample size per parameter over generations g_from..g_to of the on-device history (BDA3 section 11.5 / the Stan
 * reference manual, on the values as they are; for the rank-normalised bulk and tail ESS see demcz_rank_normalize and
 * demcz_rank_diagnostics below).  The split chains are demcz_rhat's: n = (g_to-g_from+1)/2
 * samples each, m = 2 N of them; the window needs at least 4 generations.  With c_j(t) = 1/n sum_i (x_i - mean_j)(x_{i+t} - mean_j)
 * and A(t) = 1/m sum_j c_j(t): W = A(0) n/(n-1), var+ = A(0) + sum_j (mean_j - grand)^2 / (m-1), rho_t = 1 - (W - A(t))/var+
 * (rho_0 = 1), Geyer's initial monotone sequence over the pairs P_k = rho_2k + rho_2k+1 up to lag L (n-1, or min(n-1, max_lag)
 * when max_lag > 0), tau = -1 + 2 sum P_k, ESS = m n / tau, and m n log10(m n) where tau < 1 / log10(m n).
 *
 * demcz_autocov_sums   sums[p + d*(t - lag_from)] = sum over the LOCAL 2N split chains of n*c_j(t), t = lag_from..lag_to
 *                      (0 <= lag_from <= lag_to <= n-1).  A lag's value does not depend on the other lags of the call.
 * demcz_ess_from_sums  pure host code, no device: the finisher.  sums: d x nlags from lag 0 (an unpaired last lag is ignored);
 *                      between[p] = sum_j (mean_j - grand)^2 over all m split chains (demcz_rhat_partial stage 1, out[0..d)).
 *                      pairs[p] = pairs summed; converged[p] = 1 when a pair with !(P_k > 0) ended the sequence (that pair is not
 *                      summed; a NaN pair ends it too and makes tau and ess NaN), 0 when the lags ran out: ess is then an upper
 *                      bound.  tau is returned uncapped.  Any output pointer but ess may be NULL.
 * demcz_ess            the whole statistic.  Lags are computed in batches and the finisher runs after each, until every
 *                      parameter has converged or L is reached: the cost follows the autocorrelation time, and the result is, bit
 *                      for bit, what all L lags give.  Any output pointer but ess may be NULL.  On a handle whose communicator
 *                      has more than one rank: DEMCZ_ERR_INVALID_ARGUMENT -- the sums are additive over shards; add
 *                      demcz_autocov_sums and demcz_rhat_partial over the ranks on the host and call demcz_ess_from_sums. */
int32_t demcz_autocov_sums(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t lag_from, int64_t lag_to, double* sums);
int32_t demcz_ess_from_sums(int32_t d, int64_t m, int64_t n, int64_t nlags, const double* sums, const double* between,
                            double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged);
int32_t demcz_ess(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t max_lag,
                  double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged);

/* Quantiles per parameter over generations g_from..g_to of the on-device history, by exact selection (not
 * in the reference).  All N chains and all w = g_to-g_from+1 generations are used, S = N w draws per parameter; any w >= 1.
 * Draws are ordered by the key of their bit pattern, key = bits ^ 0xFFFFFFFFFFFFFFFF when the sign bit is set and
 * bits | 1 << 63 otherwise:  -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  The quantile of probability q in [0, 1] is
 * Hyndman-Fan type 7 (np.quantile's and Julia's default): h = (double)(S-1) q, lo = floor(h) clipped to [0, S-1],
 * hi = min(lo+1, S-1), frac = h - lo, a = x_(lo), b = x_(hi) (0-based order statistics); the result is a when frac == 0 or
 * a == b and a + frac (b - a) otherwise, each operation rounded.  A parameter whose window holds a NaN is NaN in q, a and b.
 * The order statistics are found by a radix select over the key, one byte per pass from the top: eight passes, each reading
 * the window once however many probabilities were asked for.  Range and state errors are demcz_rhat's.
 *
 * demcz_quantile_plan    host code, no device: rank_lo, rank_hi, frac (nq values each) for S draws.  INVALID_ARGUMENT for nq < 1,
 *                        nq > 16, S < 1, or a probability that is NaN or outside [0, 1]; unsorted and repeated ones are fine.
 * demcz_select_counts    one counting pass over the LOCAL chains, for hosts that add over shards: for parameter p and prefix u,
 *                        counts[b + 256 (u + nprefix p)] = draws with (key >> (shift+8)) == prefix[p + d u] and
 *                        ((key >> shift) & 255) == b.  shift: a multiple of 8 in 0..56; at 56 every draw matches every prefix.
 *                        nprefix: 1..32; the prefixes of one parameter should be distinct (a draw counts towards the first it
 *                        matches).  nan_count[p] = draws with x != x (may be NULL).  The counts are integers: exact, and
 *                        additive over shards in any order.
 * demcz_select_step      host code, no device: one byte of the walk.  counts: 256 x nr x d as above with one column per rank
 *                        (already added over shards; ranks that share a prefix share its counts); for every (p, r) the first
 *                        byte whose cumulative count exceeds rank[p + d r] is appended to prefix[p + d r] (prefix << 8 | byte)
 *                        and the count below it is subtracted from the rank.  A rank not below the total of its counts:
 *                        INVALID_ARGUMENT, and nothing is written.  Start from prefix = 0, rank = the rank among all S draws;
 *                        after the pass at shift 0 the prefix is the key of the order statistic.
 * demcz_quantile_finish  host code, no device: keys back to doubles, the formula, the NaN rule.  key_lo, key_hi, q, lower, upper:
 *                        d x nq column-major; frac: nq; nan_count (d), lower and upper may be NULL.
 * demcz_quantiles        the whole statistic; q (and lower = a, upper = b unless NULL): d x nq column-major.  On a handle whose
 *                        communicator has more than one rank: DEMCZ_ERR_INVALID_ARGUMENT -- add demcz_select_counts over the
 *                        ranks on the host and step with demcz_select_step. */
int32_t demcz_quantile_plan(int64_t S, int32_t nq, const double* probs, int64_t* rank_lo, int64_t* rank_hi, double* frac);
int32_t demcz_select_counts(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t shift, int32_t nprefix,
                            const uint64_t* prefix, int64_t* counts, int64_t* nan_count);
int32_t demcz_select_step(int32_t d, int32_t nr, const int64_t* counts, uint64_t* prefix, int64_t* rank);
int32_t demcz_quantile_finish(int32_t d, int32_t nq, const uint64_t* key_lo, const uint64_t* key_hi, const double* frac,
                              const int64_t* nan_count, double* q, double* lower, double* upper);
int32_t demcz_quantiles(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nq, const double* probs,
                        double* q, double* lower, double* upper);

/* The best draw of the window (extract_best, src/utils.jl:120-125): bestval = the maximum of log_obj over generations
 * g_from..g_to, ignoring NaN (+inf can win).  Ties by == (0.0 and -0.0 tie) go to the earliest generation, then to the lowest
 * chain: the reference's column-major findn(...)[1].  chain: 0-based local chain; generation: numbered as g_from..g_to;
 * bestpar (d values, may be NULL) = chain[chain, :, generation] of the history.  When every entry is NaN, bestval is NaN, both
 * indices are -1 and bestpar is NaN.  Range and state errors are demcz_rhat's. */
int32_t demcz_best(demcz_handle* h, int64_t g_from, int64_t g_to, double* bestval, int64_t* chain, int64_t* generation,
                   double* bestpar);

/* Per-chain acceptance ratio over generations g_from..g_to:
 * sum(diff(log_obj, dims=2) .!= 0, dims=2) ./ (G-1), src/utils.jl:61.  ratio: N values. */
int32_t demcz_accept_ratio(demcz_handle* h, int64_t g_from, int64_t g_to, double* ratio);

/* mean_cov_chain over generations g_from..g_to, src/utils.jl:96-111 (1/(N*G) normalisation).
 * mean: d values, cov: d x d column-major. */
int32_t demcz_mean_cov(demcz_handle* h, int64_t g_from, int64_t g_to, double* mean, double* cov);

/* Host-closure mode (DEMCZ_TARGET_HOST_CALLBACK): one block-step of update_demcz_chain_block
 * split at the closure call demcz.jl:189.  demcz_propose draws (i1, i2, normals, log u) for
 * block ib of generation g and returns the N proposals (N x d, ld N); the caller evaluates its
 * closure; demcz_accept_commit applies demcz.jl:190-194 (tempered if temperature != NULL).
 * demcz_end_generation performs runchain!'s bookkeeping demcz.jl:84-91. */
int32_t demcz_propose(demcz_handle* h, int64_t g, int32_t ib, double gamma, double* Xprop);
/* The same round trip without its two copies and its two stream synchronisations (round 5).  demcz_closure_buffers hands out pinned
 * host buffers of the handle -- *Xprop: N x d (ld N), *logp: N -- that the kernels address directly: demcz_propose(h, g, ib, gamma,
 * NULL) returns as soon as the propose kernel has written the proposals INTO *Xprop (its last workgroup raises a flag word the host
 * spins on: no copy, no hipStreamSynchronize); the caller evaluates its closure on *Xprop, leaves the values in *logp and calls
 * demcz_accept_commit(h, NULL, temperature), which only ENQUEUES the commit (the kernel reads *logp from host memory) -- the next
 * demcz_propose goes into the stream behind it.  Do not write *logp between demcz_accept_commit and the return of the next
 * demcz_propose.  Own pointers may still be passed to either call: they are copied from / into the pinned buffers. */
int32_t demcz_closure_buffers(demcz_handle* h, double** Xprop, double** logp);
int32_t demcz_accept_commit(demcz_handle* h, const double* logp_prop, const double* temperature);
int32_t demcz_end_generation(demcz_handle* h, int64_t g);

/* Multi-GPU: one handle per rank (one process per GPU).  `unique_id` is the 128-byte
 * ncclUniqueId obtained from demcz_comm_unique_id on rank 0 and broadcast by the host
 * (torch.distributed / MPI / Distributed.jl -- plumbing).  After this call demcz_run appends
 * through ncclAllGather and demcz_rhat all-reduces its partial moments. */
int32_t demcz_comm_unique_id(void* unique_id_128B);
int32_t demcz_comm_init(demcz_handle* h, const void* unique_id_128B, int32_t nranks, int32_t rank);

/* Rows handed over INSIDE the launches (round 4).  After demcz_comm_init every rank's archive is opened by all other ranks
 * over HIP IPC (fine-grained device memory), and a rank's publisher waves store a boundary's rows into every replica themselves,
 * by write-through stores over xGMI; readers poll their own replica.  The all-gather + scatter per K-window is gone and a launch
 * runs through many K boundaries, as on one GPU: the role of the reference's shared archive under pmap (src/demcz.jl:88-91, 137),
 * without its race.  If IPC or peer access is refused on any rank, or a hand-off times out, the run falls back to the
 * ncclAllGather exchange (same results).  DEMCZ_NO_PEER=1 in the environment keeps the exchange from the start.
 *   demcz_get_peer_status   *mode = 0 exchange through RCCL (or unsharded), 1 replica group of this process, 2 IPC peers, 3 IPC peers
 *                           set up by the host (demcz_peer_export / demcz_peer_attach);
 *                           *peers = replicas this handle publishes into besides its own.
 *   demcz_peer_group        the same schedule for R handles of THIS process on ONE device (each with its own replica and shard:
 *                           chain_id0 = r * N), so that a one-GPU machine can run and test it: the members publish into each
 *                           other's replicas directly.  One host thread drives all members and gives every member the same
 *                           demcz_run calls before it asks any of them for results; demcz_run_checked is not available.
 *                           Destroying one member ends the group. */
int32_t demcz_peer_group(demcz_handle** handles, int32_t R);
int32_t demcz_get_peer_status(const demcz_handle* h, int32_t* mode, int32_t* peers);
/* The IPC set-up with the HOST carrying the 64-byte handles (torch.distributed, MPI, Distributed.jl ...) instead of RCCL -- for
 * hosts that shard without the library's communicator, and what lets two PROCESSES on one GPU test the cross-process half of the
 * path (mode 3 of demcz_get_peer_status).  demcz_peer_export moves the archive into fine-grained memory and returns its IPC
 * handle; the host all-gathers the handles; demcz_peer_attach(handles: nranks x 64 bytes in rank order) opens the others'.  The
 * host then owes two meetings of all ranks (barriers): after demcz_set_state / before the first demcz_run, and after the last
 * synchronising call / before demcz_destroy.  A hand-off that times out is DEMCZ_ERR_STATE on the rank that saw it: there is
 * no automatic redo in this mode. */
int32_t demcz_peer_export(demcz_handle* h, int32_t nranks, int32_t rank, void* handle_64B);
int32_t demcz_peer_attach(demcz_handle* h, const void* handles_64B_each);
/* The orderly end of that mode: an exported archive may only be freed once no other rank has it mapped.  After the host's
 * barrier behind the last synchronising call every rank calls demcz_peer_detach (closes its mappings of the others' archives;
 * results stay readable, demcz_run is refused from then on), the host makes the ranks meet once more, then demcz_destroy.
 * (With the library's own communicator, demcz_comm_init, demcz_destroy holds both meetings itself.) */
int32_t demcz_peer_detach(demcz_handle* h);
/* demcz_comm_init's first-contact check (round 5).  Before the in-launch hand-off is switched on, every rank's kernel stores a
 * token into every peer's archive allocation -- the store a published row uses, through the IPC mapping a row would travel --
 * while it polls its own for the peers' tokens (at most 200 ms, DEMCZ_PING_MS); the outcome and "can this rank issue LIVE
 * launches at all" are min-reduced over the ranks: either every rank hands rows over inside its launches or all of them keep
 * the ncclAllGather exchange.  *ok = 1 passed on all ranks, 0 failed somewhere (the exchange is in use), -1 not made (unsharded,
 * DEMCZ_NO_PEER, IPC refused); *wait_us = how long this rank's kernel waited for the last token (start skew + link latency). */
int32_t demcz_get_peer_ping(const demcz_handle* h, int32_t* ok, double* wait_us);

/* Deadline of every host-side wait of a sharded handle (a stream or event behind an RCCL collective): default 60 000 ms, or
 * the environment variable DEMCZ_COMM_TIMEOUT_MS at demcz_comm_init; 0 = wait for ever.  While it waits the library polls
 * ncclCommGetAsyncError about once a millisecond.  On expiry or on an asynchronous error: ncclCommAbort on the handle's
 * communicators and DEMCZ_ERR_COMM (the reference's counterpart: pmap at src/demcz.jl:137 throws when a worker dies). */
int32_t demcz_set_comm_timeout(demcz_handle* h, int64_t milliseconds);

/* Device-pointer access for hosts that do the exchange themselves (e.g. torch.distributed):
 * copy the current N x d states into caller device memory, and append `nrows` rows given as an
 * nrows x d column-major device matrix (ld = ldrows) to Z, bumping M. */
int32_t demcz_export_current_device(demcz_handle* h, double* X_device);
int32_t demcz_append_rows_device(demcz_handle* h, const double* rows_device, int64_t nrows, int64_t ldrows);
/* Host-pointer form of the append: rows is nrows x d column-major with leading dimension ldrows. */
int32_t demcz_append_rows(demcz_handle* h, const double* rows, int64_t nrows, int64_t ldrows);
/* When set (non-zero), demcz_run stops short of the K-boundary append and leaves it to the
 * caller (demcz_export_current_device + host collective + demcz_append_rows_device). */
int32_t demcz_set_external_append(demcz_handle* h, int32_t enabled);

/* Deferred visibility of appended rows.  E = 0 (default): the rows appended after generation j*K are
 * drawn from in generation j*K + 1 already -- the reference's schedule with all chains of a
 * generation updated against the same archive.  E >= 1: boundaries are grouped in batches of E
 * (batch of boundary j closes at J = ceil(j/E)*E) and a batch's rows are drawn from generation
 * (J + E)*K + 1 on.  On a sharded handle the batch travels in ONE all-gather on a side stream while
 * the next E windows compute, so the latency-bound collective is off the critical path; on an
 * unsharded handle the same rule is applied so results do not depend on the sharding.  Any past
 * state is a legitimate DEMCz archive row (ter Braak & Vrugt 2008); this changes WHEN a row becomes
 * eligible, not the target distribution.  Call after demcz_comm_init, before demcz_run. */
int32_t demcz_set_append_lag(demcz_handle* h, int32_t batches);

/* Resume: the chains' Philox streams have already been advanced by `generations` generations (the
 * length of a previous run, demcz.jl:18-22): generation g of this handle draws what generation
 * generations+g of an uninterrupted run would draw.  K boundaries still follow this handle's own g,
 * like the reference's restarted `ig`. */
int32_t demcz_set_rng_offset(demcz_handle* h, int64_t generations);

/* Snooker generations: the second updater of DE-MCzs (ter Braak & Vrugt 2008).  Off by default.  With every = s >= 1,
 * generation g is a snooker generation when (g + rng_offset) % s == 0 -- the number that positions the Philox streams, so a
 * resumed run (demcz_set_rng_offset) makes the choices an uninterrupted one would.  In a snooker generation every chain makes
 * ONE step on all d parameters, whatever the block structure, in place of the generation's block-steps: it jumps along the line
 * from an archive row a through its state x, x' = x + gamma_s ((z1 - z2) . e / e . e) e with e = x - a, z1, z2, a three distinct
 * archive rows, gamma_s ~ U(gamma_lo, gamma_hi), and accepts with log u < (logp(x') - logp(x)) / T + (d - 1)/2 log(|x' - a|^2 /
 * |x - a|^2); a step whose |x - a|^2 or |x' - a|^2 is not a positive normal double is rejected (DESIGN.md section 3 has the
 * arithmetic, operation by operation).  History, changed counts and the K-boundary append are those of any generation.  A
 * snooker generation is a launch of its own (snooker_kernel); demcz_run, demcz_run_checked, caller-owned appends
 * (demcz_set_external_append) and the RCCL exchange work as before.  The paper's choice: every = 10, (1.2, 2.2).
 * May be called after demcz_create and again between runs (every = 0 switches off).
 * DEMCZ_ERR_INVALID_ARGUMENT: every < 0; bounds not finite or not 0 < gamma_lo <= gamma_hi; d < 2; the handle was not created
 * on the one-lane layout (lanes_per_chain = 1 -- the other layouts draw ahead of the chains).  DEMCZ_ERR_STATE: a host-callback
 * handle, a derived history, a handle in a replica group or with IPC peers.  demcz_run with snooker generations on and fewer
 * than three archive rows returns DEMCZ_ERR_STATE before anything is enqueued. */
int32_t demcz_set_snooker(demcz_handle* h, int32_t every, double gamma_lo, double gamma_hi);
/* What was set, and the snooker launches made in the handle's life (any pointer may be NULL). */
int32_t demcz_get_snooker(const demcz_handle* h, int32_t* every, double* gamma_lo, double* gamma_hi, int64_t* steps_launched);

/* Crossover generations: the subspace sampling and the multi-pair jump of DREAM(ZS) (Vrugt et al. 2009; Laloy & Vrugt 2012).
 * Off by default (ncr = 0 switches off).  With ncr >= 1 every generation that is not a snooker generation is a crossover
 * generation: every chain makes ONE step with ONE log-density evaluation, in which it draws a CR class m with the integer
 * weights (P(m) = w_m / W), a number of pairs delta ~ U{1 .. delta_max}, and moves a random subset of its parameters -- each
 * selected with probability (m + 1) / ncr, one at random if none was -- by
 *   x'_p = x_p + (gamma / sqrt(2 delta d') (sum over delta pairs of Z[i1, p] - Z[i2, p]) + eps_p z_p),   d' = the subset's size;
 * the other parameters keep their bits.  Accept rule, temperature, history, changed counts and the K-boundary append are those
 * of any generation.  A generation takes S_cr = 1 + delta_max + ceil(d / 4) + ceil(d / 2) + 1 Philox blocks of the chain's
 * stream, at fixed positions (DESIGN.md section 3 has the arithmetic, word by word); a snooker generation reads the first three
 * of them.  weights: ncr values >= 0 whose sum W has 1 <= W < 2^31, or NULL for all 1.
 * DEMCZ_ERR_INVALID_ARGUMENT: ncr outside 0 ... 8; delta_max outside 1 ... 3; a negative weight or W outside [1, 2^31); d < 2;
 * more than one block; a handle not created on the one-lane layout (lanes_per_chain = 1).  DEMCZ_ERR_STATE: a host-callback
 * handle, a derived history, a handle in a replica group or with IPC peers, and a handle that has already run a generation
 * (the stride positions the streams: a resumed run sets crossover on the fresh handle, before demcz_set_rng_offset).
 * demcz_run with crossover on and fewer than two archive rows returns DEMCZ_ERR_STATE before anything is enqueued;
 * demcz_peer_group and demcz_propose refuse such a handle. */
int32_t demcz_set_crossover(demcz_handle* h, int32_t ncr, const int32_t* weights, int32_t delta_max);
/* What was set, and per CR class the steps tried and those whose accept test was true, summed over the handle's life (snooker
 * generations are not counted).  weights: ncr values; tried, accepted: 8 values each.  Any pointer may be NULL.  Synchronises
 * the handle's stream when counts are asked for -- and, on a handle with demcz_set_crossover_adapt, when the weights are: they are
 * the device's then. */
int32_t demcz_get_crossover(const demcz_handle* h, int32_t* ncr, int32_t* weights, int32_t* delta_max, int64_t* tried, int64_t* accepted);

/* Adaptation of the CR class weights during burn-in, on the device (DREAM's rule, Vrugt et al. 2009 section 3; DESIGN.md section
 * 3).  Off by default (every = 0 switches off), and with it off nothing changes.  With it on, every crossover step at a position
 * g + rng_offset <= until adds 1 to its class's `tried` and, when accepted, the squared jump distance -- every parameter's move
 * times the reciprocal standard deviation of that parameter over the handle's chains (rsd), summed -- to its class's `dist`,
 * quantised to 1/65536 and clamped at 65536.  Behind every generation with (g + rng_offset) % every == 0 up to `until` the weights
 * become w_k = max(min_weight, (int32)(r_k / R * 65536)) with r_k = dist_k / tried_k and R their sum (unchanged while R = 0), and rsd
 * is computed again; the sums are cumulative from the start of adaptation.  Behind `until` the weights are frozen.  The positions are
 * in the stream numbering, as the snooker rule's: a resumed run adapts where an uninterrupted one would.  Nothing here synchronises:
 * the weights live on the device and launches are cut at the update positions.  demcz_get_crossover then reports the device's weights.
 * until: a multiple of every; min_weight: 1 ... 8192 (656 is 1 % of 65536); N * until < 2^31 (else DEMCZ_ERR_INVALID_ARGUMENT).
 * DEMCZ_ERR_STATE: crossover is off; the handle has already run a generation; the handle appends externally
 * (demcz_set_external_append: a shard's own chains are not the population -- such drivers set weights by hand with
 * demcz_set_crossover_weights; demcz_set_external_append in turn refuses an adapting handle).  demcz_set_crossover with ncr = 0 or a
 * changed ncr clears the adaptation. */
int32_t demcz_set_crossover_adapt(demcz_handle* h, int64_t every, int64_t until, int32_t min_weight);
/* The setting and the state: weights, dist, tried: 8 values each (dist in units of 1/65536); rsd: d values; updates made so far.
 * Any pointer may be NULL.  Synchronises the handle's stream. */
int32_t demcz_get_crossover_adapt(const demcz_handle* h, int64_t* every, int64_t* until, int32_t* min_weight, int32_t* weights,
                                  int64_t* dist, int64_t* tried, double* rsd, int64_t* updates);
/* The other half of a checkpoint: what demcz_get_crossover_adapt returned, onto a fresh handle with the adaptation set (after
 * demcz_set_crossover and demcz_set_crossover_adapt; with demcz_set_rng_offset the run then continues as the uninterrupted one).
 * The spread is then not computed at the first demcz_run.  The arrays are read, not written (dist and tried are `int64_t*` as
 * demcz_get_crossover_adapt's are, so that one pair of buffers serves both calls from any binding). */
int32_t demcz_set_crossover_adapt_state(demcz_handle* h, const int32_t* weights, int64_t* dist, int64_t* tried, const double* rsd,
                                        int64_t updates);
/* New weights for a crossover handle in mid-life (ncr values, as demcz_set_crossover's: >= 0, 1 <= W < 2^31): the stride of the
 * streams does not depend on them.  They hold from the next launch on.  DEMCZ_ERR_STATE on a handle without crossover, and while the
 * adaptation is still running: as long as the last generation run lies in front of `until`, g_done + rng_offset < until.  (In an
 * uninterrupted run, and in one resumed with demcz_set_crossover_adapt_state, that is updates * every < until; a handle resumed
 * behind `until` without the state is past its adaptation by position and is not refused.) */
int32_t demcz_set_crossover_weights(demcz_handle* h, const int32_t* weights);

/* Stateless diagnostics on caller (host) arrays, for code that post-processes returned histories
 * the way the reference's examples do (test/example_normpdf.jl:35-47): the array is uploaded, reduced
 * on the device, and nothing is kept.
 *   demcz_rhat_array          Rhat_gelman(chain, N, G, d)              src/utils.jl:2-20
 *   demcz_accept_ratio_array  sum(diff(log_obj,dims=2).!=0,dims=2)./(G-1)   src/utils.jl:61
 *   demcz_mean_cov_array      mean_cov_chain(chain, N, G, d)           src/utils.jl:96-111
 *   demcz_autocov_sums_array / demcz_ess_array   the two calls above over the whole array (not in the reference)
 *   demcz_quantiles_array     demcz_quantiles over the whole array (not in the reference)
 *   demcz_best_array          demcz_best over an N x G log_obj; column: 0-based              src/utils.jl:120-125 */
int32_t demcz_rhat_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, double* rhat);
int32_t demcz_accept_ratio_array(int32_t device_id, const double* log_obj, int64_t N, int64_t G, double* ratio);
int32_t demcz_mean_cov_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, double* mean, double* cov);
int32_t demcz_autocov_sums_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G,
                                 int64_t lag_from, int64_t lag_to, double* sums);
int32_t demcz_ess_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t max_lag,
                        double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged);
int32_t demcz_quantiles_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nq,
                              const double* probs, double* q, double* lower, double* upper);
int32_t demcz_best_array(int32_t device_id, const double* log_obj, int64_t N, int64_t G, double* bestval, int64_t* chain,
                         int64_t* column);

/* Derived quantities (generated quantities; not in the reference): m user-written functions of every draw of a history window,
 * evaluated on the device into a DERIVED HISTORY -- a second handle that holds nothing but the N x m x w values and takes every
 * statistic above unchanged, so that a variance from a log-variance, a contrast of two coefficients or the indicator x[0] > 0
 * (whose mean is a probability) is summarised without the history leaving the device.  A derive program is HIP C++ that defines
 *     __device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out);
 * x: the DEMCZ_D (= d of the source) parameters of one draw; logp: its log_obj, NaN where the source keeps none (arrays given
 * without log_obj, a derived history); data: the ndata doubles given with the program (device memory, read-only; NULL when
 * ndata is 0); out: DEMCZ_M (= m) entries, preset to NaN -- an entry the function does not write stays NaN.  DEMCZ_D, DEMCZ_M,
 * INFINITY and NAN are defined for the program.  Compiled like a program target: --offload-arch=gfx950 -O3 -ffp-contract=off
 * -I<rocm>/include, then `options` (space-separated, may be NULL); a fused multiply-add happens only where fma() is written.
 * The unit holds the program and one streaming kernel (one lane per draw), none of the library's window kernels, and shares the
 * process-wide cache of program targets under a key of its own that includes m.  1 <= d <= 32, 1 <= m <= 32.
 * The function is called once per draw in no particular order, so it must be a pure function of its arguments.  Indexing x or
 * out with a run-time value sends those arrays to scratch memory; loops over the compile-time DEMCZ_D and DEMCZ_M unroll and
 * keep them in registers.
 *   demcz_derive_check  compiles the program and needs no device.  DEMCZ_OK, or DEMCZ_ERR_INVALID_ARGUMENT with the compiler log
 *                       (user's line numbers, file "program") in demcz_last_error(NULL); d or m out of range: the same code with a
 *                       message that names the limit.
 *   demcz_derive        generations g_from..g_to of h's history (range and state errors are demcz_rhat's; a voided LIVE slab is
 *                       redone first).  The program is compiled or taken from the cache and loaded on h's device, data copied to
 *                       memory the derived history owns, the kernel run on h's stream behind what is queued there, and the call
 *                       returns when it is done.  A compile error is DEMCZ_ERR_INVALID_ARGUMENT with the log in
 *                       demcz_last_error(h); a failed allocation DEMCZ_ERR_HIP, nothing leaked.  *derived is NULL on every
 *                       failure.  Works on a sharded handle and on a member of a replica group: the map is per draw, local to
 *                       the handle's own chains.
 *   demcz_derive_array  the same from host arrays: chain N x d x G column-major, log_obj N x G or NULL; generations 1..G.  The
 *                       uploads are freed before it returns; only the derived history stays.
 * The derived history is a demcz_handle with N chains, m "parameters" and w = g_to-g_from+1 generations that KEEP THEIR NUMBERS:
 * the statistics are asked for g_from..g_to or any window inside.  It owns its memory, outlives the handle it came from and is
 * freed by demcz_destroy.  It takes demcz_rhat, demcz_rhat_partial, demcz_autocov_sums, demcz_ess, demcz_select_counts,
 * demcz_quantiles, demcz_mean_cov, demcz_get_history with log_obj = NULL, demcz_synchronize, demcz_last_error, demcz_destroy,
 * demcz_derive (a derived history of a derived history; its logp is NaN), demcz_predict, demcz_ppc and demcz_rank_normalize, demcz_indicator_le,
 * demcz_rank_diagnostics, demcz_histogram, demcz_histogram2d, demcz_hdi, demcz_pointwise, demcz_loo_columns, demcz_loo and (a one-column one, as either argument)
 * demcz_bridge_iterate (below).  Every other call that takes a handle returns
 * DEMCZ_ERR_STATE on it, with a message that says so. */
int32_t demcz_derive_check(int32_t d, int32_t m, const char* source, const char* options);
int32_t demcz_derive(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                     const double* data, int64_t ndata, demcz_handle** derived);
int32_t demcz_derive_array(int32_t device_id, const double* chain, const double* log_obj /* may be NULL */,
                           int64_t N, int32_t d, int64_t G, int32_t m, const char* source, const char* options,
                           const double* data, int64_t ndata, demcz_handle** derived);

/* Posterior predictive programs (not in the reference): a derive program that is also given random numbers, so that a replicated
 * data set y_rep ~ p(y | theta), a predictive draw at a new covariate or a posterior predictive p-value is computed where the
 * history lies.  A predictive program is HIP C++ that defines
 *     __device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out);
 * with x, logp, data, out, DEMCZ_D, DEMCZ_M, the compile options, the limits 1 <= d, m <= 32 and the advice on run-time indices
 * exactly demcz_derive's, and rng the draw's own random stream, consumed through
 *     void   demcz_bits(demcz_rng*, uint64_t* r1, uint64_t* r2)   the next 128 bits of the stream
 *     double demcz_uniform(demcz_rng*)                            in (0, 1)
 *     double demcz_normal(demcz_rng*)                             standard normal (Box-Muller)
 *     double demcz_exponential(demcz_rng*)                        -log(uniform)
 * THE STREAM OF A DRAW (DESIGN.md section 3 has the specification to the bit): the draw of global chain c = chain_id0 + local
 * chain at generation g owns the Philox4x32-10 stream of key `seed` and subsequence (g << 32) | c.  What a draw is given therefore
 * depends on (seed, g, c) and on nothing else: not on the window asked for, the launch, how the chains are sharded over handles
 * or demcz_set_history_origin; a call repeated is the same bits, and a draw may consume as many numbers as it likes.  With the
 * run's own seed these streams cannot meet the sampler's or the bridge's, whose subsequences are chain numbers below 2^32 while
 * g >= 1 puts these at 2^32 and above.  Two programs run with one seed are given the same numbers: give them different seeds
 * where their results must be independent.  seed and chain_id0 are the caller's to give; nothing is read off the handle.  Needs
 * g_to < 2^32 and 0 <= chain_id0, chain_id0 + N <= 2^32 (DEMCZ_ERR_INVALID_ARGUMENT otherwise).
 *   demcz_predict_check  compiles the program and needs no device; errors as demcz_derive_check's.
 *   demcz_predict        the program at every draw of generations g_from..g_to of h's history: a DERIVED HISTORY (see demcz_derive)
 *                        of m columns.  Range, state, refusals, the voided LIVE slab and the error codes are demcz_derive's; h may
 *                        be a derived history (its logp is NaN).
 *   demcz_predict_array  the same from host arrays, generations 1..G.
 *   demcz_ppc            the same calls of the program, but no history is written: out[k] of every draw is compared with
 *                        observed[k] (m values; NULL: zeros) and counts[3 k], [3 k + 1], [3 k + 2] return how many draws had
 *                        out[k] > observed[k], out[k] == observed[k], and out[k] NaN.  A posterior predictive p-value of the
 *                        statistic T is (gt + eq) / (N w - nan) with out[k] = T(y_rep, theta) and observed[k] = T(y, theta), or
 *                        with out[k] their difference and observed NULL.  Integer counts: the same bits however the window is
 *                        cut or the chains are sharded, and the counts of shards add.  A NaN observed[k] counts every draw in
 *                        neither gt nor eq.  Nothing is leaked on any failure.
 *   demcz_ppc_array      the same from host arrays, generations 1..G. */
int32_t demcz_predict_check(int32_t d, int32_t m, const char* source, const char* options);
int32_t demcz_predict(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                      const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, demcz_handle** derived);
int32_t demcz_predict_array(int32_t device_id, const double* chain, const double* log_obj /* may be NULL */,
                            int64_t N, int32_t d, int64_t G, int32_t m, const char* source, const char* options,
                            const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, demcz_handle** derived);
int32_t demcz_ppc(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                  const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, const double* observed /* m, or NULL: zeros */,
                  int64_t* counts /* 3 m: gt, eq, nan of each column */);
int32_t demcz_ppc_array(int32_t device_id, const double* chain, const double* log_obj /* may be NULL */,
                        int64_t N, int32_t d, int64_t G, int32_t m, const char* source, const char* options,
                        const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, const double* observed /* m, or NULL: zeros */,
                        int64_t* counts /* 3 m */);

/* Rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; not in the reference): rank-normalised split
 * R-hat, bulk-ESS and tail-ESS, from the exact average rank of every draw among all S = N w draws of its parameter (DESIGN.md
 * sections 3 and 4.14).  Per parameter p the value ranked is v = x (center NULL: bulk) or fabs(x - center[p]) (folded), then
 * v + 0.0, so that -0.0 ranks as +0.0: ties are ties by ==, +-inf rank like any other value.  The average rank is
 * r = less + (equal + 1) / 2 (1-based; less: draws with a smaller v, equal: draws with the same v, itself included), the normal
 * score z = PPND16(u) (Wichura's AS 241) with Blom's u = (r - 0.375) / (S + 0.25), formed from the nearer end: z(S + 1 - r) is
 * -z(r) to the bit.  A parameter whose window holds a NaN is NaN in every entry; the other parameters are unaffected.
 *   demcz_rank_to_z           z[i] of average rank r[i] among S draws (1 <= r[i] <= S < 2^50): host code, no device -- the operation
 *                             sequence the kernel runs, bit for bit.
 *   demcz_rank_normalize      generations g_from..g_to of h's history into a DERIVED HISTORY (see demcz_derive) of N chains, d columns
 *                             and generations that keep their numbers: the normal scores (DEMCZ_RANK_Z) or the average ranks
 *                             themselves (DEMCZ_RANK_AVERAGE, the input of rank plots).  It takes every call a derived history
 *                             takes; h may be a derived history itself.  Range and state errors are demcz_rhat's; a voided LIVE slab
 *                             is redone first.  The sort works in 2 S d words of device memory that are returned before the call
 *                             ends; a failed allocation is DEMCZ_ERR_HIP, nothing leaked.  *ranked is NULL on every failure.
 *                             At most 2^31 - 1 draws per parameter.
 *   demcz_indicator_le        the derived history of the d nthr columns out[c, p + d u, g] = (x[c, p, g] <= thr[p + d u]) ? 1 : 0; a NaN
 *                             draw stays NaN.  1 <= nthr <= 64.  A map per draw: works on a sharded handle.
 *   demcz_rank_diagnostics    rhat_rank = max(R-hat of the bulk scores, R-hat of the scores folded at the type-7 median), NaN if
 *                             either is; ess_bulk = demcz_ess of the bulk scores; ess_tail = the smaller demcz_ess of the
 *                             indicators x <= q(0.05) and x <= q(0.95) (type-7 quantiles, demcz_quantiles), NaN if either is.
 *                             d values each; any may be NULL but not all.  The window needs at least 4 generations.
 *   ..._array                 the same from a host array N x d x G column-major, generations 1..G.
 * A rank needs the draws of every shard, and unlike the quantiles' counts there is no additive shard protocol for it here: on a
 * handle whose communicator has more than one rank demcz_rank_normalize and demcz_rank_diagnostics return
 * DEMCZ_ERR_INVALID_ARGUMENT -- gather the window with demcz_get_history and use the _array form. */
#define DEMCZ_RANK_Z 0        /* normal scores */
#define DEMCZ_RANK_AVERAGE 1  /* the average ranks themselves (rank plots) */
int32_t demcz_rank_to_z(int64_t n, const double* r, int64_t S, double* z);
int32_t demcz_rank_normalize(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t mode,
                             const double* center /* d values or NULL */, demcz_handle** ranked);
int32_t demcz_rank_normalize_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G,
                                   int32_t mode, const double* center, demcz_handle** ranked);
int32_t demcz_indicator_le(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nthr,
                           const double* thr /* d x nthr */, demcz_handle** derived);
int32_t demcz_rank_diagnostics(demcz_handle* h, int64_t g_from, int64_t g_to,
                               double* rhat_rank, double* ess_bulk, double* ess_tail);
int32_t demcz_rank_diagnostics_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G,
                                     double* rhat_rank, double* ess_bulk, double* ess_tail);

/* Posterior densities (not in the reference beyond the 33-bin histogram its convergence_check once drew): marginal histograms,
 * pairwise histograms and highest-density intervals over generations g_from..g_to of the history on the device (DESIGN.md
 * sections 3 and 4.18).  Counts are integers: exact, bit-reproducible, additive over shards in any order.
 *
 * THE BIN RULE.  Parameter p has nbins uniform bins over [lo[p], hi[p]] with the edge table
 *     edges[p][k] = numpy.linspace(lo[p], hi[p], nbins + 1)[k]:   k * ((hi - lo) / nbins) + lo, two rounded operations after the
 *     division (should (hi - lo) / nbins underflow to 0: (k / nbins) * (hi - lo) + lo), and edges[p][nbins] = hi exactly.
 * A draw x lies in bin k iff edges[k] <= x < edges[k+1]; the last bin also takes x == edges[nbins].  x < edges[0] (-inf too)
 * counts in below[p], x > edges[nbins] (+inf too) in above[p], a NaN in nan_count[p].  -0.0 compares as 0.0.  The table decides,
 * not the rounding of any estimate: the counts are numpy.histogram(x, bins = nbins, range = (lo, hi))'s.
 *   demcz_histogram_edges  host code, no device: the table of one parameter, nbins + 1 values.  INVALID_ARGUMENT unless
 *                          1 <= nbins <= 4096 and lo < hi, both finite, hi - lo finite -- and unless the table comes out
 *                          non-decreasing, which it does between normal doubles (a span of a few thousand subnormals can fail).
 *   demcz_histogram        counts: d x nbins, [p][k] (row-major); edges: d x (nbins + 1), [p][k], the tables used (may be NULL);
 *                          below, above, nan_count: d values each (any may be NULL).  lo, hi: d values each, or both NULL: the
 *                          AUTOMATIC RANGE, the window's smallest and largest draw of the parameter (exact: demcz_quantiles at
 *                          probabilities 0 and 1); where the two are equal, (x - 0.5, x + 0.5).  A parameter whose extreme is NaN
 *                          or infinite: INVALID_ARGUMENT, the message names the parameter -- give a range.  A given range must be
 *                          finite with lo < hi for every parameter.  On a handle whose communicator has more than one rank the
 *                          counts are those of the handle's own chains: give the range, and add the counts over the ranks.
 *   demcz_histogram2d      npairs pairs (p, q) = (pairs[2 i], pairs[2 i + 1]), p != q, both in 0..d-1; p's draws go by its table
 *                          of nbx bins, q's by its table of nby bins, both over the parameter's range [lo, hi] (d values each, or
 *                          both NULL as above).  counts: npairs x nbx x nby, [i][kx][ky]; a draw with either coordinate outside
 *                          its range, or NaN, counts in outside[i] (may be NULL) and in no cell:
 *                          numpy.histogram2d(x_p, x_q, bins = [edges_x[p], edges_y[q]]).  1 <= nbx, nby <= 128: the 32-bit counters
 *                          of one pair are then at most the 64 KB of LDS a workgroup may have.  edges_x: d x (nbx + 1), edges_y:
 *                          d x (nby + 1) (may be NULL).  At most 2^27 cells in one call.
 *   demcz_hdi_steps        host code, no device: steps[j] = min(floor(probs[j] S), S - 1) for 1 to 16 probabilities inside (0, 1).
 *   demcz_hdi              the shortest interval between two order statistics that spans m = demcz_hdi_steps steps: with s the
 *                          window's S = N w draws of the parameter in ascending order (-0.0 taken as 0.0),
 *                          i* = argmin over 0 <= i < S - m of s[i + m] - s[i], one rounded subtraction each; ties go to the
 *                          smallest i; a NaN width (inf - inf) is never a candidate.  hdi: d x nprob x 2, [p][j][0] = s[i*],
 *                          [p][j][1] = s[i* + m]; NaN, NaN without a candidate, and for a parameter with a NaN draw in the window.
 *                          The sort is demcz_rank_normalize's, in 2 S d words of device memory returned before the call ends; at
 *                          most 2^31 - 1 draws per parameter.  On a handle whose communicator has more than one rank:
 *                          INVALID_ARGUMENT -- the sort is of one handle's draws; gather the window and use demcz_hdi_array.
 *   ..._array              the same from a host array N x d x G column-major, generations 1..G.
 * Range and state errors are demcz_rhat's; h may be a derived history. */
int32_t demcz_histogram_edges(int32_t nbins, double lo, double hi, double* edges);
int32_t demcz_histogram(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nbins, const double* lo, const double* hi,
                        double* edges, int64_t* counts, int64_t* below, int64_t* above, int64_t* nan_count);
int32_t demcz_histogram_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nbins,
                              const double* lo, const double* hi, double* edges, int64_t* counts, int64_t* below,
                              int64_t* above, int64_t* nan_count);
int32_t demcz_histogram2d(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t npairs, const int32_t* pairs, int32_t nbx,
                          int32_t nby, const double* lo, const double* hi, double* edges_x, double* edges_y,
                          int64_t* counts, int64_t* outside);
int32_t demcz_histogram2d_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t npairs,
                                const int32_t* pairs, int32_t nbx, int32_t nby, const double* lo, const double* hi,
                                double* edges_x, double* edges_y, int64_t* counts, int64_t* outside);
int32_t demcz_hdi_steps(int64_t S, int32_t nprob, const double* probs, int64_t* steps);
int32_t demcz_hdi(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nprob, const double* probs, double* hdi);
int32_t demcz_hdi_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nprob,
                        const double* probs, double* hdi);

/* PSIS-LOO and WAIC (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024; the generalised-Pareto fit of
 * Zhang & Stephens 2009; not in the reference): how well the model predicts each observation it was fitted to, from the history
 * on the device (DESIGN.md sections 3 and 4.16).  Three layers, each with an entry point of its own.
 *
 * 1. Pointwise log-likelihoods.  A pointwise program is HIP C++ that defines
 *     __device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i);
 * the log-likelihood of observation i at the draw x[0..DEMCZ_D), a pure function of its arguments.  It is compiled like a derive
 * program (same options, same caches; DEMCZ_D, INFINITY and NAN are defined) into a unit with one streaming kernel: a lane loads
 * its draw once and walks the observations of the chunk, whose bounds are the same in every lane.  1 <= d <= 32.
 *   demcz_pointwise_check  compiles the program and needs no device; errors as demcz_derive_check's.
 *   demcz_pointwise        observations obs_from .. obs_from + mc - 1 (1 <= mc <= 32; the caller keeps them below its number of
 *                          observations) at every draw of generations g_from..g_to: a DERIVED HISTORY (see demcz_derive) of mc
 *                          columns whose generations keep their numbers.  Refusals and error codes are demcz_derive's.
 *   demcz_pointwise_array  the same from a host array N x d x G column-major; generations 1..G.
 *
 * 2. demcz_loo_columns treats the d columns of h's history -- a sampling handle, a derived history -- as the log-likelihoods a of d
 * observations over the window's S = N w draws, each column on its own.  With the column sorted, a_0 <= a_1 <= ..., and
 * lw_j = a_0 - a_j: M = ceil(min(S / 5, 3 sqrt(S / r_eff))) (r_eff: d values in (0, inf), or NULL for 1); the cutoff
 * c = max(lw_M, log DBL_MIN); the tail the n elements with lw > c, strictly (ties at the cutoff shorten it); for n >= 5 the
 * generalised-Pareto fit of the exceedances exp(lw) - exp(c) gives k and sigma, and the tail's weights are replaced by the
 * fit's quantiles, capped at 0.  Outputs, d values each, any may be NULL:
 *   elpd_loo   log sum exp(lw' + a) - log sum exp(lw')          pareto_k   (n k + 5) / (n + 10); +inf where n < 5 or k is not finite
 *   n_tail     n                                                 lppd       log mean exp(a)
 *   p_waic     the sample variance of a, divisor S - 1 (NaN at S = 1)
 * A column with a NaN or an infinite entry is NaN in every output with n_tail 0; the other columns are unaffected.  A constant
 * column gives n_tail 0, pareto_k +inf, elpd_loo = lppd = the constant and p_waic 0.  No floating-point atomics: the same call
 * gives the same bits, and a column's results do not depend on the columns beside it.  Range and state errors are demcz_rhat's;
 * like demcz_rank_normalize it sorts in 2 S d words of scratch, takes at most 2^31 - 1 draws per column and refuses a handle
 * whose communicator has more than one rank.  demcz_loo_columns_array: the same from a host array N x d x G.
 *   demcz_psis_tail_length  *M of S draws: host code, no device.
 *   demcz_gpd_fit           k, sigma and the regularised khat of n >= 5 exceedances in ascending order: host code, no device,
 *                           the per-term functions of the kernel with the sums in index order.
 *
 * 3. demcz_loo: the outputs above for observations 0..nobs-1 of a pointwise program, in chunks of observations -- demcz_pointwise,
 * demcz_loo_columns, the chunk dropped -- of the largest width <= 32 whose scratch (24 bytes per draw and observation) fits
 * 4 GiB.  r_eff: nobs values or NULL.  The results are demcz_loo_columns's of the same columns, bit for bit.  demcz_loo_array: the
 * same from a host array.  The relative efficiency of an observation is not computed here: demcz_ess of demcz_pointwise's
 * history gives it. */
int32_t demcz_pointwise_check(int32_t d, const char* source, const char* options);
int32_t demcz_pointwise(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t obs_from, int32_t mc, const char* source,
                        const char* options, const double* data, int64_t ndata, demcz_handle** derived);
int32_t demcz_pointwise_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t obs_from,
                              int32_t mc, const char* source, const char* options, const double* data, int64_t ndata,
                              demcz_handle** derived);
int32_t demcz_psis_tail_length(int64_t S, double r_eff, int64_t* M);
int32_t demcz_gpd_fit(int64_t n, const double* x_ascending, double* k, double* sigma, double* khat);
int32_t demcz_loo_columns(demcz_handle* h, int64_t g_from, int64_t g_to, const double* r_eff /* NULL or d values */,
                          double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic);
int32_t demcz_loo_columns_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, const double* r_eff,
                                double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic);
int32_t demcz_loo(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t nobs, const char* source, const char* options,
                  const double* data, int64_t ndata, const double* r_eff /* NULL or nobs values */,
                  double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic);
int32_t demcz_loo_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t nobs,
                        const char* source, const char* options, const double* data, int64_t ndata, const double* r_eff,
                        double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic);

/* The marginal likelihood log Z = log integral exp(logobj(x)) dx by bridge sampling (the optimal bridge of Meng & Wong 1996; the
 * iterative scheme of Gronau et al. 2017; the error estimate of Fruehwirth-Schnatter 2004; not in the reference), from the history
 * on the device (DESIGN.md sections 3 and 4.17).  It gives Bayes factors and posterior model probabilities.  It assumes that
 * log_obj is the untempered log-posterior of the draws (not an annealing run) and that the window is converged; a posterior far
 * from normal shows as a large se_logml and a slow iteration.  Four layers, each with an entry point of its own; 1 <= d <= 32.
 *
 * The window g_from..g_to of w >= 4 generations is cut at h = floor(w / 2): generations g_from .. g_from + h - 1 fit the proposal
 * g = N(m, L L^T) -- (m, V) is demcz_mean_cov of them, L the lower Cholesky factor of V computed on the host; a pivot that is not
 * positive and finite is DEMCZ_ERR_INVALID_ARGUMENT with the parameter's index in the message -- and generations g_from + h .. g_to
 * are the N1 = N (w - h) posterior draws of the iteration.  mean: d values; L: d x d column-major, its lower triangle is read.
 *
 * 1. demcz_bridge_posterior: a1 = log_obj - log g(x) of every draw of generations g_from..g_to of h, by the solve L z = x - m: a
 * one-column DERIVED HISTORY (see demcz_derive) whose generations keep their numbers.  A derived history as h has no log_obj:
 * DEMCZ_ERR_STATE.  demcz_bridge_posterior_array: the same from host arrays N x d x G and N x G; generations 1..G.
 *
 * 2. demcz_bridge_proposal: Np x wp fresh draws of g -- draw j = c + Np t takes its normals from Philox blocks t B .. t B + B - 1,
 * B = ceil(d / 2), of stream (seed, chain c), the pairs demcz_selftest_draws returns -- and a2 = logobj(x) - log g(x) with the
 * handle's own target, built-in or program (a program's bridge unit is compiled on first use): *logratio is a one-column derived
 * history of generations 1..wp; with draws != NULL, *draws is the Np x d x wp derived history of the draws themselves.  A NaN from
 * the target stays NaN.  A host-closure handle has no target on the device and is refused (DEMCZ_ERR_STATE).
 * demcz_bridge_proposal_program: the same for a program (demcz_set_program's source, options and data) without a handle.
 * demcz_bridge_check compiles a program's bridge unit and needs no device; errors as demcz_program_check's.
 *
 * 3. demcz_bridge_iterate works on any two one-column histories on one device: a1 over generations g_from..g_to of post (N1
 * values), a2 over gp_from..gp_to of prop (N2 values).  With s1 = neff / (neff + N2), s2 = 1 - s1 (neff <= 0 means N1),
 *     f1_j = 1 / (s1 + s2 exp(rho - a2_j))   f2_i = 1 / (s1 exp(a1_i - rho) + s2)   rho' = rho + log mean f1 - log mean f2
 * from rho_0 = max a1, until |rho' - rho| <= tol (*converged = 1) or max_iter updates (>= 1) have been made.  *logml is the last
 * rho', *iterations the number of updates.  A NaN in a2 counts as -inf and is counted in *n_nan.  A non-finite a1, a +inf in a2
 * or a mean that is 0 gives *logml = NaN with *converged = 0 (and NaN moments).  moments[4] = mean f1, var f1, mean f2, var f2 at
 * the final rho, variances with divisor n.  With f2 != NULL, *f2 is f2 at the final rho as a derived history numbered as post's
 * window.  Sums are made in tiles of 1024 added in index order, without floating-point atomics: the same call gives the same
 * bits, and neither they nor *iterations depend on how many updates are queued between two synchronisations (4; the environment
 * variable DEMCZ_BRIDGE_BATCH, 1..64, sets another number).
 *
 * 4. demcz_bridge: the whole pipeline on h's history with Np = N, wp = w - h.  Outputs, any may be NULL: logml; se_logml =
 * sqrt(var f1 / (N2 mean f1^2) + var f2 / (ess_f2 mean f2^2)); iterations; converged; n_post = N1; n_prop = N2; neff_used; n_nan;
 * ess_f2 = demcz_ess of f2 over the iteration window (NaN, and se_logml with it, where that window has fewer than 4 generations);
 * mean_out (d) and L_out (d x d column-major) of the proposal.  Use a seed
 * other than the run's: with the run's own the proposal would replay the sampler's streams.  demcz_bridge_array: the same from
 * host arrays and a program.  Range and state errors are demcz_rhat's; a handle whose communicator has more than one rank is
 * refused as demcz_rank_normalize refuses it (gather the window and use demcz_bridge_array).  Every failure leaves the derived
 * histories NULL. */
int32_t demcz_bridge_check(int32_t d, const char* source, const char* options);
int32_t demcz_bridge_posterior(demcz_handle* h, int64_t g_from, int64_t g_to, const double* mean, const double* L,
                               demcz_handle** derived);
int32_t demcz_bridge_posterior_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d,
                                     int64_t G, const double* mean, const double* L, demcz_handle** derived);
int32_t demcz_bridge_proposal(demcz_handle* h, int64_t Np, int64_t wp, uint64_t seed, const double* mean, const double* L,
                              demcz_handle** logratio, demcz_handle** draws /* may be NULL */);
int32_t demcz_bridge_proposal_program(int32_t device_id, int32_t d, int64_t Np, int64_t wp, uint64_t seed, const double* mean,
                                      const double* L, const char* source, const char* options, const double* data,
                                      int64_t ndata, demcz_handle** logratio, demcz_handle** draws /* may be NULL */);
int32_t demcz_bridge_iterate(demcz_handle* post, int64_t g_from, int64_t g_to, demcz_handle* prop, int64_t gp_from,
                             int64_t gp_to, double neff, double tol, int64_t max_iter, double* logml, int64_t* iterations,
                             int32_t* converged, double* moments /* 4 values */, int64_t* n_nan,
                             demcz_handle** f2 /* may be NULL */);
int32_t demcz_bridge(demcz_handle* h, int64_t g_from, int64_t g_to, uint64_t seed, double neff, double tol, int64_t max_iter,
                     double* logml, double* se_logml, int64_t* iterations, int32_t* converged, int64_t* n_post,
                     int64_t* n_prop, double* neff_used, int64_t* n_nan, double* ess_f2, double* mean_out, double* L_out);
int32_t demcz_bridge_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d, int64_t G,
                           const char* source, const char* options, const double* data, int64_t ndata, uint64_t seed,
                           double neff, double tol, int64_t max_iter, double* logml, double* se_logml, int64_t* iterations,
                           int32_t* converged, int64_t* n_post, int64_t* n_prop, double* neff_used, int64_t* n_nan,
                           double* ess_f2, double* mean_out, double* L_out);

/* Introspection for benchmarks and tests. */
int32_t demcz_get_info(const demcz_handle* h, int64_t* M, int64_t* launches_window, int32_t* lanes_per_chain);

/* The driver loop with its autostop test as ONE call (demcz.jl:30-55): generations g_from..g_to, and after
 * every generation g that is a multiple of `every` the split-R-hat of generations (g-every, g]
 * (Rhat_gelman, utils.jl:2-20; demcz.jl:41).  The maximum over parameters of the i-th check goes to
 * rhat_max[i] (i < n_max; may be NULL), the whole vector of the last check to rhat_last[d] (may be NULL).
 * threshold > 0: returns as soon as a check's maximum is below it, with *g_stop = that generation
 * (demcz.jl:43-52; the state is as if nothing after it had run -- the library may run the next slab ahead of the
 * decision and discards it); otherwise *g_stop = g_to.  *n_checks = checks made.
 * Needs a history window (Gcap) that holds the generations of the call.  In a sharded run every rank
 * makes the same call; the decision is the same on all of them.                                      */
int32_t demcz_run_checked(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature,
                          int64_t every, double threshold, int64_t* g_stop, int32_t* n_checks,
                          double* rhat_max, int32_t n_max, double* rhat_last);

/* ------------------------------------------------------------------------------------------------------
 * DIAGNOSTIC entry points -- NOT part of the drop-in contract; a binding of the reference
 * surface needs none of them.  They exist for bench.py (kernel timing), for tests (self-test of the draw
 * arithmetic, forcing the LIVE hand-off's time-out path) and for integrators who want to look inside.
 * ------------------------------------------------------------------------------------------------------ */

/* Timing of the window kernels on the stream they are launched on: while enabled, every demcz_run call
 * brackets its back-to-back window launches with one HIP event pair (an event between two launches would
 * stall the stream being measured).  demcz_get_kernel_time synchronises, returns the number of window
 * launches covered and the summed duration of the brackets, and clears the record.                     */
int32_t demcz_set_kernel_timing(demcz_handle* h, int32_t enabled);
int32_t demcz_get_kernel_time(demcz_handle* h, int64_t* launches, double* milliseconds);

/* The brackets the last demcz_get_kernel_time call summed up, one per demcz_run call (inside demcz_run_checked: one per slab):
 * start_ms[i] = start of bracket i on the device clock, relative to the first bracket's start; duration_ms[i] = its length.
 * start_ms[i+1] - start_ms[i] is therefore the wall time of step i as the GPU saw it, gaps between launches included -- what
 * bench.py takes its median step time from.  At most `cap` entries are written; *n = entries available.
 * demcz_run_checked with threshold <= 0 may run k consecutive slabs as one demcz_run call with one bracket: that bracket is
 * returned as k entries, start + i * duration / k and duration / k -- means over the launch, not events.  demcz_get_kernel_time
 * keeps returning the true launch count and the summed bracket time. */
int32_t demcz_get_kernel_time_series(demcz_handle* h, int32_t cap, double* start_ms, double* duration_ms, int32_t* n);

/* Device self-test of the draw pipeline: for Philox block blk0+i of the
 * stream of global chain `chain`, words[2i..2i+1] = the two raw 64-bit words,
 * normals[2i..2i+1] = the Box-Muller pair, logu[i] = log(u_open(word 0)).  Lets an integrator
 * check the device arithmetic against any host implementation of the spec, bit for bit. */
int32_t demcz_selftest_draws(int32_t device_id, uint64_t seed, uint64_t chain, uint64_t blk0, int32_t n,
                             uint64_t* words, double* normals, double* logu);

/* LIVE launches (split layout on one GPU: a launch runs through many K boundaries and its waves hand the appended
 * rows to each other through the archive itself).  A wave that polls `polls` times for a row without seeing it
 * gives up; the library then redoes everything since the last verified point with one launch per K-window
 * (results are bit-identical either way).  polls = 0 restores the default (2^18).
 * demcz_get_live_status: *live_enabled = 1 while the handle issues LIVE launches, *redos = times it had to
 * fall back.  Tests lower the limit to 1 to walk the fall-back path.
 * Re-arming (round 5).  A time-out is not for ever: the redo runs one launch per K-window up to and including the demcz_run
 * call (inside demcz_run_checked: the slab) that holds the generation whose row never arrived, and the first call behind it
 * issues LIVE launches again -- in a sharded run on every rank together (the ranks agree on the point through the reduced error
 * words, and on "can go LIVE again" through one more reduction).  A handle does this at most `n` times in its life (default 3;
 * DEMCZ_LIVE_REARMS in the environment at demcz_create; demcz_set_live_rearms), after which a failure leaves it at one launch
 * per K-window, the mode that cannot fail.  demcz_get_live_rearms: *rearms = times it went LIVE again, *left = what remains. */
int32_t demcz_set_live_spin_limit(demcz_handle* h, int32_t polls);
int32_t demcz_get_live_status(const demcz_handle* h, int32_t* live_enabled, int32_t* redos);
int32_t demcz_set_live_rearms(demcz_handle* h, int32_t n);
int32_t demcz_get_live_rearms(const demcz_handle* h, int32_t* rearms, int32_t* left);
/* Diagnostic: window launches so far by the kernel that took them (three values): counts[0] window_kernel_ps2 (the regular
 * launches of the wave-per-chain layout), [1] that layout's general kernels (window_kernel_ps / _pw), [2] launches of every
 * other layout.  Tests use it to know which kernel a parity case exercised. */
int32_t demcz_debug_kernel_counts(const demcz_handle* h, int64_t* counts);
/* Diagnostic: the name (template arguments included, as a profiler prints it) of the window kernel the handle's most recent
 * window launch ran, NUL-terminated into buf[cap].  bench.py labels its roofline objects with it. */
int32_t demcz_debug_kernel_name(const demcz_handle* h, char* buf, int32_t cap);

/* Fault injection for the LIVE hand-off: LIVE launches whose first generation is >= g_from use the poll limit `polls` instead
 * of the handle's (demcz_set_live_spin_limit), so that a test can make a hand-off fail LATE in a long call (e.g. in slab 280 of
 * a 300-slab demcz_run_checked).  polls = 0 switches it off; a fault that has fired (the redo it caused has rolled back) switches
 * itself off, so that the redo's own LIVE launches run undisturbed.  polls = -1: such a launch finds the error word already set -- as if
 * a wave had timed out before the others became resident (another process on the GPU) -- so every wave leaves at once; the redo
 * snapshot buffers are filled with NaN patterns beforehand, so a wave that left without writing its row of the snapshot shows. */
int32_t demcz_debug_set_live_fault(demcz_handle* h, int32_t polls, int64_t g_from);

/* Fault injection for the exchange: the next collective of this (sharded) handle is held back on its stream for `milliseconds`
 * (at most 10 000; a one-thread kernel that watches a host flag and the clock, so it always ends) -- to a waiting rank exactly
 * what a stalled peer looks like.  Lets a one-GPU box walk the deadline -> abort -> DEMCZ_ERR_COMM path. */
int32_t demcz_debug_stall_exchange(demcz_handle* h, int32_t milliseconds);

/* The scatter step of the sharded K-boundary exchange on caller data: `slab` (host) has the layout an all-gather
 * over R ranks delivers, [R][cnt][d][n_loc] doubles with n_loc = the handle's N; its R*cnt*n_loc rows are appended
 * in the order an unsharded run appends them (boundary, then rank, then chain).  batched = 0: the kernel of the
 * synchronous exchange (cnt must be 1); 1: the kernel of the batched one.  Lets a one-GPU machine check the R > 1
 * index arithmetic that otherwise only runs behind ncclAllGather on R GPUs. */
int32_t demcz_debug_append_slab(demcz_handle* h, const double* slab, int32_t R, int32_t cnt, int32_t batched);

#ifdef __cplusplus
}
#endif
#endif /* DEMCZ_H */
