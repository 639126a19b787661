// demcz_capi.hip -- the C ABI of include/demcz.h over the kernels of demcz_kernels.h.
// Host side of the seam src/demcz.jl:30-33 / src/demcz_anneal.jl:39-42 (see the header).
// There is no CPU fallback: without a HIP device every entry point fails with
// DEMCZ_ERR_NO_DEVICE.
#include "../../include/demcz.h"
#include "demcz_kernels.h"
#include "demcz_kernels_acf.h"
#include "demcz_kernels_sel.h"
#include "demcz_select_host.h"
#include "demcz_kernels_rank.h"
#include "demcz_kernels_density.h"
#include "demcz_kernels_loo.h"
#include "demcz_kernels_bridge.h"
#include "demcz_slab_plan.h"
#include "demcz_run_plan.h"
#include "demcz_kernels_ml.h"
#include "demcz_kernels_pc.h"
#include "demcz_kernels_lr.h"
#include "demcz_kernels_ps.h"
#include "demcz_kernels_ps2.h"
#include "demcz_kernels_ps2d.h"
#include "demcz_kernels_snooker.h"
#include "demcz_kernels_crossover.h"
#include "demcz_pw_dispatch.h"
#include "demcz_mlr_dispatch.h"
#include "demcz_program.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <cstdlib>
#include <deque>
#include <map>
#include <mutex>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using namespace demcz;

static thread_local std::string g_create_error;

// ---- buffer pools ---------------------------------------------------------------------------------------------------------
// The reference's demcz_sample allocates its result arrays per call (demcz.jl:24); behind this ABI that is a device history, an
// archive and -- for the streamed history -- pinned host mirrors of half a gigabyte at C2, per call.  hipMalloc / hipFree /
// hipHostMalloc of that size cost milliseconds each (and hipFree synchronises the device), so buffers a destroyed handle gives
// back are kept (up to a cap) for the next handle of the process: a second demcz_sample call allocates nothing.
namespace {
struct BufPool {
    struct Entry { void* p; size_t bytes; int device; };
    std::mutex mu;
    std::vector<Entry> free_list;
    size_t cached = 0;
    const size_t cap;
    const bool host;
    BufPool(size_t cap_, bool host_) : cap(cap_), host(host_) {}
    hipError_t acquire(void** out, size_t bytes, int device)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            int best = -1;
            for (int i = 0; i < (int)free_list.size(); ++i) {
                const Entry& e = free_list[i];
                if (e.device == device && e.bytes >= bytes && e.bytes <= bytes + bytes / 4 + (1u << 20) && (best < 0 || e.bytes < free_list[best].bytes)) best = i;
            }
            if (best >= 0) {
                *out = free_list[best].p;
                cached -= free_list[best].bytes;
                sizes[*out] = free_list[best].bytes;
                free_list.erase(free_list.begin() + best);
                return hipSuccess;
            }
        }
        hipError_t e = host ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes);
        if (e != hipSuccess) {
            // what this pool keeps for later may be exactly what is missing now (a handle of another shape, another library of
            // the process): give everything cached back to the runtime and ask once more
            (void)hipGetLastError();
            if (trim() > 0) e = host ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes);
        }
        if (e == hipSuccess) { std::lock_guard<std::mutex> lk(mu); sizes[*out] = bytes; }
        return e;
    }
    // frees every cached buffer; returns the bytes given back
    size_t trim()
    {
        std::vector<Entry> drop;
        size_t n = 0;
        {
            std::lock_guard<std::mutex> lk(mu);
            drop.swap(free_list);
            n = cached;
            cached = 0;
        }
        for (const Entry& e : drop) { if (host) (void)hipHostFree(e.p); else (void)hipFree(e.p); }
        return n;
    }
    // a buffer something may still be writing (an undrained stream, an aborted communicator's kernels): never cached -- hipFree /
    // hipHostFree wait for the device
    void discard(void* p)
    {
        if (!p) return;
        { std::lock_guard<std::mutex> lk(mu); sizes.erase(p); }
        if (host) (void)hipHostFree(p); else (void)hipFree(p);
    }
    void release(void* p, int device)
    {
        if (!p) return;
        size_t bytes = 0;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = sizes.find(p);
            if (it != sizes.end()) { bytes = it->second; sizes.erase(it); }
            if (bytes && cached + bytes <= cap && !getenv("DEMCZ_NO_POOL")) {
                free_list.push_back({p, bytes, device});
                cached += bytes;
                return;
            }
        }
        if (host) (void)hipHostFree(p); else (void)hipFree(p);
    }
    std::unordered_map<void*, size_t> sizes;
};
BufPool g_dev_pool(6ull << 30, false);      // device buffers (history, archive arena): at most 6 GiB kept
BufPool g_host_pool(3ull << 30, true);      // pinned host mirrors of the history: at most 3 GiB kept
}  // namespace
// ... and so are its streams (creating and destroying five streams was 4-5 ms of an end-to-end C2 call)
static std::mutex g_stream_mu;
static std::vector<std::pair<int, hipStream_t>> g_stream_pool;
static hipError_t stream_acquire(int device, hipStream_t* out)
{
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        for (size_t i = 0; i < g_stream_pool.size(); ++i)
            if (g_stream_pool[i].first == device) { *out = g_stream_pool[i].second; g_stream_pool.erase(g_stream_pool.begin() + (long)i); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void stream_release(int device, hipStream_t s, bool drained)
{
    if (!s) return;
    if (drained && !getenv("DEMCZ_NO_POOL")) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        if (g_stream_pool.size() < 32) { g_stream_pool.emplace_back(device, s); return; }
    }
    (void)hipStreamDestroy(s);
}
// every device / pinned allocation of a handle goes through the pools (a pointer the pool does not know is simply freed)
static hipError_t dev_malloc(int device, void** out, size_t bytes) { return g_dev_pool.acquire(out, std::max<size_t>(bytes, 16), device); }
static hipError_t dev_free(int device, void* p) { g_dev_pool.release(p, device); return hipSuccess; }
static hipError_t host_malloc(void** out, size_t bytes) { return g_host_pool.acquire(out, std::max<size_t>(bytes, 16), -1); }
static hipError_t host_free(void* p) { g_host_pool.release(p, -1); return hipSuccess; }

struct demcz_handle;
// The consumer of a handle in the split layout (lanes == DEMCZ_LAYOUT_SPLIT): who reads the draw records
enum SplitKind {
    SPLIT_NONE = 0,   // not the split layout
    SPLIT_PC8,        // eight replicated lanes per chain (window_kernel_pc8)
    SPLIT_ML,         // sixteen cooperating lanes per chain (window_kernel_ml / _lr16 / _lr8s, REC)
    SPLIT_MLB,        // cooperating lanes with block updates (window_kernel_mlb, REC)
    SPLIT_WAVE,       // one wave per chain, speculating (window_kernel_ps / _ps2 / _ps2d / _pw, or the program's own)
};

// One window launch's kernel, as window_kernel_of() resolves it: everything that launches, sizes, counts or names a window kernel
// reads this description and decides nothing about the instantiation itself.
enum KernelArm { ARM_ONE_LANE, ARM_ML, ARM_ML_COOP, ARM_MLB, ARM_LR16, ARM_PC8, ARM_ML_REC, ARM_MLB_REC, ARM_LR16_REC, ARM_LR8S,
                 ARM_PS, ARM_PS2, ARM_PS2D, ARM_PW, ARM_PROGRAM_WAVE, ARM_SNOOKER, ARM_CROSSOVER };
struct WindowKernel {
    const void* fn = nullptr;       // host symbol of a built-in kernel ...
    hipFunction_t mod = nullptr;    // ... or the function of the program's module; neither: not built (or no program yet)
    int threads = 0;                // per workgroup
    size_t dyn_lds = 0;             // dynamic LDS bytes
    bool big_lds = false;           // ... which may exceed the default limit (launch_kernel / blocks_per_cu raise it)
    int waves = 0;                  // split layout: waves of a workgroup (each runs chains or producer units); fused layouts: its chain waves
    bool steady = false;            // the steady-state kernel (window_kernel_ps2 / _ps2d): counted in kernel_counts[0]
    // what demcz_debug_kernel_name prints it from
    KernelArm arm = ARM_ONE_LANE;
    bool live = false, temper = false;
    int pw_form = 0;                // ARM_PW: PW_FORM_*
    bool adapt = false;             // ARM_CROSSOVER: the ADAPT instantiation, with its third kernel argument
};

// What window_kernel_of() is told about one launch, beside the handle's own layout
struct LaunchFacts {
    bool live = false;        // the launch runs through K boundaries (or has peers): the LIVE instantiation
    bool temper = false;      // tempered accept
    bool ps2 = false;         // ps2_applicable(h, P)
    bool dual = false;        // h->dual_now
    bool pw_reg = false;      // pw_regular(P, live)
    bool pw_matrix = false;   // pw_matrix_form(h)
    bool coop = false;        // ml_coop(h)
    bool lr16 = false;        // uses_lr16(h)
    bool snooker = false;     // the launch is one snooker generation (LaunchPlan::snooker)
    bool crossover = false;   // the launch's generations are crossover generations (demcz_set_crossover; not a snooker launch)
    bool adapt = false;       // ... of a handle with demcz_set_crossover_adapt: the ADAPT instantiation, for life
};

// A replica group of one process (demcz_peer_group): R handles on one device, each with its own archive replica and shard of
// the chains, publishing boundary rows into each other's replicas from inside their launches.  One host thread drives them all.
struct PeerGroup {
    std::vector<demcz_handle*> members;
    bool failed = false;       // a hand-off timed out: calls are logged and executed in lockstep at the next verification ...
    int32_t rearms_left = 3;   // ... after which the group tries its in-launch hand-off again, this many times in its life
    bool lockstep_only = false;   // a layout without the hand-off, or streams that cannot run at the same time: never LIVE
    bool busy = false;         // inside group_verify / group_execute
    bool dead = false;         // a member was destroyed: the others only accept demcz_destroy
};

struct demcz_handle {
    demcz_config cfg{};
    int lanes = 1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // host copies of the small tables
    std::vector<int32_t> block_offsets, block_indices, slot_of;
    std::vector<double> eps;
    int64_t S = 0;            // Philox blocks per generation
    int64_t ZS = 0;           // archive row stride in doubles (row-major on the device)
    bool full_block = false;
    int ngrp = 1;             // MvNormal: groups the sums of the quadratic form are cut into (TargetParams::ngrp; 1 = not grouped)
    uint64_t gstart = 1ull;   // bit j: parameter j starts a group
    int mlb_qb = 0;           // > 0: the groups are equal blocks of this many parameters and the block kernel's incremental form is built for them
    // device buffers
    double* dZ = nullptr;
    double* dX = nullptr;
    double* dlp = nullptr;
    double* dchain = nullptr;
    double* dchain_alloc = nullptr;   // what the pool gave (dchain may sit a few bytes into it: DEMCZ_DEBUG_HIST_SKEW)
    double* dlogobj = nullptr;
    double* dlp_origin = nullptr;   // log_obj of every chain when the history window opened
    bool origin_valid = false;
    double* dtemp = nullptr;
    int64_t temp_cap = 0;
    int32_t* d_block_offsets = nullptr;
    int32_t* d_slot_of = nullptr;
    double* d_eps = nullptr;
    double* d_mu = nullptr;
    double* d_Wp = nullptr;
    double* d_design = nullptr;
    double* d_y = nullptr;
    // scratch for reductions
    double* d_scratch = nullptr;
    int64_t scratch_cap = 0;
    double* d_stage = nullptr;     // host-visible staging for small results / uploads
    int64_t stage_cap = 0;
    // state
    int64_t M = 0;
    int64_t g_done = 0;
    int64_t g0 = 0;           // history origin
    int64_t rng_offset = 0;   // generations already consumed from every chain's stream (resume)
    bool has_state = false;
    int64_t launches = 0;
    mutable int64_t kernel_counts[1] = {0};               // demcz_debug_kernel_counts: launches taken by window_kernel_ps2
    WindowKernel last_kernel;         // demcz_debug_kernel_name: what the most recent window launch ran (threads == 0: none yet)
    bool external_append = false;
    // host-closure mode
    double* dXprop = nullptr;
    double* dlogu = nullptr;
    bool proposal_pending = false;
    bool gen_open = false;
    // host-closure mode, pipelined (round 5: demcz_closure_buffers).  Proposals and their log-densities live in pinned host memory
    // the kernels address directly: propose_kernel writes the N x d proposals there (and the device copy the commit needs), the
    // last workgroup to finish raises a flag word in the same memory, the host spins on the flag -- no D2H copy, no stream
    // synchronisation; accept_commit_kernel reads the N log-densities straight from host memory and is only ENQUEUED: the next
    // demcz_propose goes into the stream behind it while it runs.
    double* hc_X = nullptr;           // pinned, mapped: N x d (ld N)
    double* hc_lp = nullptr;          // pinned, mapped: N
    volatile unsigned int* hc_flag = nullptr;   // pinned, mapped: [0] = sequence number of the last proposal that is complete in hc_X
    unsigned int* hc_count = nullptr; // device: workgroups of the current propose launch that have finished
    unsigned int hc_seq = 0;
    // split layout: draw records, double-buffered (this launch reads one, its producer half fills the other)
    hipStream_t diag_stream = nullptr;   // demcz_run_checked, monitoring: the checks run here beside the next slab
    hipEvent_t diag_ev = nullptr;
    hipEvent_t rhat_side_ev = nullptr;   // behind the latest check enqueued on a side stream (they all work in d_scratch) ...
    bool rhat_side_pending = false;      // ... which a check on the compute stream has to wait for
    double* d_spec_X = nullptr;       // demcz_run_checked with a threshold: state before the slab enqueued ahead of a decision
    double* d_spec_lp = nullptr;
    hipEvent_t spec_ev = nullptr;
    double* pinned_rhat = nullptr;    // demcz_run_checked: pinned host slots the checks' results are copied to
    unsigned int* pinned_err = nullptr;       // demcz_run_checked: the hand-off's error word, copied behind the call's last launch ...
    int64_t pinned_err_launches = -1;         // ... valid while no window launch has been made since (h->launches then)
    int64_t pinned_cap = 0;
    bool timing = false;              // demcz_set_kernel_timing: events around every window-kernel launch
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timed;
    std::vector<int32_t> timed_slabs;    // autostop slabs each bracket covers (demcz_run_checked groups them; 1 otherwise)
    std::vector<double> series_start_ms, series_dur_ms;     // of the brackets the last demcz_get_kernel_time summed up
    int64_t timed_launches = 0;
    int64_t live_wg_cap = -1;         // consumer workgroups a LIVE launch may have (all must be resident at once); -1: not asked yet
    SplitKind split_kind = SPLIT_NONE;   // lanes == DEMCZ_LAYOUT_SPLIT: the consumer
    int split_lanes = 0;              // SPLIT_ML, SPLIT_MLB: lanes per chain of the consumer
    int split_per_wg = 1;             // chains per consumer workgroup
    int32_t* d_slot_role = nullptr;   // SPLIT_MLB: role of every Philox block of a generation
    double* d_rec[2] = {nullptr, nullptr};
    unsigned int* d_live_err = nullptr;   // device word a LIVE launch sets when an expected row never appears
#ifdef DEMCZ_STAMPS
    unsigned long long* d_stamps = nullptr;
#endif
    // wave-per-chain layout, d <= 5: archive, both record buffers and the launch's temperatures in ONE allocation (dZ), chain
    // and log_obj histories in one too -- what window_kernel_ps2 needs to address everything with 32-bit offsets
    bool arena = false, rec_in_arena = false, hist_joint = false;
    int64_t arena_gens = 0;           // generations each record buffer of the arena holds
    int64_t arena_span = 0;           // generations a LIVE launch of the arena may cover (demcz_slab_plan.h: arena_span)
    double* arena_rec[2] = {nullptr, nullptr};
    double* arena_temp = nullptr;
    int64_t rec_cap = 0;              // generations each buffer holds
    int rec_cur = 0;
    bool host_paced = false;          // inside demcz_run_checked (a blocking call): see launch_window_pc
    int wpw = 1;                      // waves per consumer workgroup of the lane-cooperative kernels (window_kernel_ml / _mlb): 1 or 4, by population
    bool ps_dual = false;             // SPLIT_WAVE, d <= 5: two chains to a wave in regular launches (window_kernel_ps2d)
    bool dual_now = false;            // ... and the launch being prepared is one of those
    bool lr_spec = false;             // SPLIT_ML, regression target: window_kernel_lr8s (eight chains per workgroup, two generations per pass)
    bool no_live = false;             // a LIVE hand-off failed on this handle: one launch per K-window from then on
    bool live_claimed = false;        // this handle holds its device's LIVE slot (one handle per device at a time)
    unsigned int live_spin_limit = 0; // polls before a LIVE wait gives up (0: the default, demcz_kernels_rec.h)
    int32_t live_fault_polls = 0;     // demcz_debug_set_live_fault: this poll limit instead of live_spin_limit ...
    int64_t live_fault_g = 0;         // ... in launches that start at this generation or later (0 polls: off)
    bool in_checked = false;          // inside demcz_run_checked: the call verifies (and, if need be, redoes) itself as a whole
    // LIVE launches are verified at the next synchronising call; until then the state they started from and the
    // calls made since are kept, so that a failed hand-off is redone with one launch per K-window (live_verify)
    struct RunCall { int64_t g_from, g_to; double gamma; bool tempered; std::vector<double> temperature; };
    std::vector<RunCall> live_log;
    double* d_safe_X = nullptr;
    double* d_safe_lp = nullptr;
    bool snap_pending = false;     // the state copy into d_safe_* is still to be made: by the next launch itself, or in front of it
    int64_t safe_M = 0, safe_M_app = 0, safe_g_done = 0;
    bool replaying = false;
    int32_t live_redos = 0;
    // Re-arming (round 5): a failed hand-off no longer costs the handle its LIVE launches for good.  live_rollback notes the
    // generation whose row never arrived; the redo runs one launch per K-window up to and including the demcz_run call that
    // holds that generation, and the first call that starts behind it goes LIVE again (live_try_rearm) -- at most
    // `live_rearms_left` times in the handle's life (default 3, DEMCZ_LIVE_REARMS, demcz_set_live_rearms), so that a handle
    // whose hand-off fails every time (another process's kernels on the GPU, a link that delays rows for good) still ends in
    // the one-launch-per-K-window mode that cannot fail.
    int32_t live_rearms_left = 3;
    int32_t live_rearms = 0;          // times the handle went LIVE again
    int64_t rearm_from = -1;          // >= 0: a demcz_run call that starts behind this generation re-arms (no_live is set)
    uint32_t fail_row_hint = 0xffffffffu;   // archive row of the wait that failed (live_failed -> live_rollback), 0xffffffff: unknown
    RecDesc rec_desc[2];              // what each draw-record buffer holds (demcz_run_plan.h)
    // wave-per-chain split layout: the producer half of a launch is a kernel of its own on a side stream (its own, small
    // register budget: it fills the SIMDs beside the one-wave-per-SIMD consumers instead of sharing their workgroup shape)
    hipStream_t prod_stream = nullptr;
    hipEvent_t prod_done[2] = {nullptr, nullptr};   // records of buffer b are complete
    hipEvent_t prod_gate = nullptr;                 // main stream: the consumer that last read the buffer about to be refilled is done
    bool prod_pending[2] = {false, false};          // buffer b was (or is being) filled on the side stream: wait for prod_done[b]
    // An event (not owned here) recorded on the compute stream after the most recent window launch, nullptr if there is none:
    // whoever needs "that launch is done" on another stream -- the R-hat stream, the producer gate of the next launch --
    // waits for it instead of putting a marker of its own into the stream.  (Every marker between two window launches is
    // microseconds of an idle GPU: scripts/step_overhead.py.)
    hipEvent_t after_launch_ev = nullptr;
    // accept mask by ballot: per launch and consumer wave {changed over the launch, changed in its first generation};
    // a ring of launches, newest last (demcz_get_changed_total)
    unsigned int* d_acc = nullptr;
    int64_t acc_waves = 0;            // consumer waves of a window launch of this handle's layout
    int32_t acc_slots = 0, acc_next = 0;
    struct LaunchRec { int64_t g_first, g_last; int32_t slot; };
    std::deque<LaunchRec> acc_log;
    // multi-GPU
    ncclComm_t comm = nullptr;          // collectives on the compute stream: synchronous all-gather, R-hat all-reduces
    ncclComm_t comm_side = nullptr;     // its duplicate (ncclCommSplit) for the batched all-gathers on the side stream: operations
                                        // of ONE communicator are serialised by RCCL whatever stream they are enqueued on
    int nranks = 1, rank = 0;
    double* d_gather = nullptr;
    // deferred visibility of appended rows (demcz_set_append_lag): M counts the rows proposals may
    // draw from, M_app the rows written or reserved; equal when lag == 0
    int lag = 0;
    int64_t M_app = 0;
    struct PendingRows { int64_t visible_from; int64_t M_after; hipEvent_t ev; int64_t xseq = 0; };   // xseq: the exchange that carries the rows (0: none yet)
    std::deque<PendingRows> pending;
    int64_t batch_J = -1;              // boundary index that closes the batch the last pending entry belongs to
    // sharded + lag: snapshots of a batch travel together on a side stream
    hipStream_t comm_stream = nullptr;
    double* d_send[2] = {nullptr, nullptr};
    double* d_recv[2] = {nullptr, nullptr};
    hipEvent_t buf_done[2] = {nullptr, nullptr};
    // exchanges are numbered; the compute stream already waits for exchange number `xseq_waited` and everything before it
    // (admit_pending), so a send buffer last read by one of those needs no wait of its own
    int64_t xseq = 0, xseq_waited = 0, buf_xseq[2] = {0, 0};
    int batch_buf = 0, batch_cnt = 0;
    int64_t batch_base = 0;
    // streamed history (demcz_history_stream): pinned host mirrors of chain / log_obj, filled slab by slab on a copy stream while
    // the next slab computes
    bool hs_on = false;
    double* hs_chain = nullptr;
    double* hs_logobj = nullptr;
    hipStream_t hs_stream = nullptr;
    bool pooled_dev = false;           // dZ / dchain came from (and go back to) the process-wide device pool
    // comm failure path: every host-side wait of a sharded handle has a deadline (demcz_set_comm_timeout); on expiry, or on an
    // asynchronous RCCL error, both communicators are aborted and the handle is dead (DEMCZ_ERR_COMM from every call)
    // exchanges completed on the side stream, written by a one-thread kernel behind each batch's scatter into pinned host memory:
    // what a host-paced wait polls (hipEventQuery of an event recorded behind a stream-wait was seen to report "complete" while
    // the work in front of it had not run -- tests/test_gpu_comm_failure.py, lag 2 -- so the host does not ask the runtime)
    volatile long long* xdone = nullptr;
    // Replicated archives with the rows handed over inside the launches (demcz_kernels_rec.h, live_publish): 0 = off; 1 = a
    // replica group of handles of THIS process on one device (demcz_peer_group: rehearsal of the schedule on a one-GPU box);
    // 2 = the ranks of the RCCL communicator, every rank's archive opened over IPC by all others (demcz_comm_init)
    int peer_mode = 0;
    int n_peers = 0;
    double* peer_Z[DEMCZ_MAX_PEERS] = {nullptr};
    void* ipc_mapped[DEMCZ_MAX_PEERS] = {nullptr};   // mode 2: what hipIpcOpenMemHandle returned (closed at destroy)
    struct PeerGroup* group = nullptr;               // mode 1
    bool err_clean = false;            // the LIVE error word was read as zero and no LIVE launch has been enqueued since
    bool peer_fence = false;           // mode 2: the ranks must meet before the next launch that publishes into peers (this
                                       // replica's unwritten rows were just re-filled with the sentinel: set_state, rollback)
    unsigned int* d_err_all = nullptr; // mode 2: [0] max over ranks of the LIVE error word, [1] barrier scratch
    bool archive_fine = false;         // dZ is a fine-grained allocation of its own (hipExtMallocWithFlags), not the pool's
    size_t dZ_bytes = 0;
    size_t mailbox_off = 0;            // archive_fine: byte offset of the 4 KiB mailbox behind the archive (peer_ping)
    bool peers_closed = false;         // mode 3: demcz_peer_detach has closed the mappings of the peers' archives (no further demcz_run)
    int32_t ping_ok = -1;              // demcz_comm_init's first-contact check: -1 not made, 0 failed (on some rank), 1 passed on all
    double ping_wait_us = 0.0;         // ... and how long THIS rank waited for the last peer's token
    int64_t live_share = 0;            // per-mille of the device's LIVE capacity this handle holds (live_claim)
    int64_t comm_timeout_ms = 60000;
    bool comm_dead = false;
    int* stall_flag = nullptr;         // device word; demcz_debug_stall_exchange: the stall kernel spins until it is set
    int32_t stall_next_ms = 0;
    // program target (demcz_set_program): the loaded module of the program's kernels; its data live in d_design, ndata in
    // cfg.nobs (the TargetParams slots only the regression reads)
    bool prog_ready = false;
    demcz_prog::Module prog;
    std::string prog_source, prog_options;   // the program's text, for the units compiled later (demcz_bridge: UNIT_BRIDGE)
    // created with DEMCZ_LAYOUT_PROGRAM_WAVE: lanes == DEMCZ_LAYOUT_SPLIT, split_kind == SPLIT_WAVE, and the consumer is the program's own
    // window_kernel_ps / _pw<TARGET_PROGRAM, d, LIVE, TEMPER> (prog.fn[WAVE_KERNEL ..]); records, producer, LIVE machinery: the library's
    bool prog_wave = false;
    // a derived history (demcz_derive): N x cfg.d x cfg.Gcap values in dchain, the program's data in d_design, a stream, the
    // staging buffer and nothing else -- no state, no archive, no log_obj.  The statistics over dchain and demcz_derive itself
    // take it; every other entry point refuses it (NOT_DERIVED) before it looks at a buffer that is not there.
    bool derived = false;
    // snooker generations (demcz_set_snooker; one-lane handles): every snooker_every-th generation of the stream numbering is one
    // snooker step on all d parameters, gamma_s ~ U(snooker_lo, snooker_hi); 0: off
    int64_t snooker_every = 0;
    double snooker_lo = 1.2, snooker_hi = 2.2;
    int64_t snooker_steps = 0;        // snooker launches made in the handle's life
    bool snooker_now = false;         // the launch being prepared is one (LaunchPlan::snooker)
    // crossover generations (demcz_set_crossover; one-lane handles with one block): every generation that is not a snooker
    // generation is one crossover step of every chain; cr_ncr == 0: off.  While it is on, S is crossover_stride(d, cr_delta_max)
    // (S_plain keeps the stride of the block structure).
    int32_t cr_ncr = 0, cr_delta_max = 1;
    int32_t cr_weights[CR_MAX_CLASSES] = {1, 1, 1, 1, 1, 1, 1, 1};
    unsigned long long* d_cr_counts = nullptr;      // [workgroup][8][2], zeroed when crossover is switched on
    int64_t S_plain = 0;
    // adaptation of the class weights during burn-in (demcz_set_crossover_adapt): cr_adapt_every == 0: off.
    // The state lives on the device, in one block (CRA_*): the kernels read and write it with no host in between.
    int64_t cr_adapt_every = 0, cr_adapt_until = 0;
    int32_t cr_adapt_min_weight = 656;
    unsigned char* d_cr_adapt = nullptr;
    bool cr_adapt_started = false;    // rsd has been computed (the first demcz_run) or restored (demcz_set_crossover_adapt_state)
    bool cr_accumulate_now = false;   // the launch being prepared lies at or in front of `until`
};

// the block behind demcz_handle::d_cr_adapt, in bytes: weights[8] (int32), cum[8] (uint32), updates (int64), rsd[MAX_D], slots[nwg][8][2]
constexpr size_t CRA_WEIGHTS = 0, CRA_CUM = 32, CRA_UPDATES = 64, CRA_RSD = 128, CRA_SLOTS = CRA_RSD + 8 * MAX_D;
static size_t cra_workgroups(const demcz_handle* h) { return (size_t)((h->cfg.N + WINDOW_BS - 1) / WINDOW_BS); }
static size_t cra_bytes(const demcz_handle* h) { return CRA_SLOTS + cra_workgroups(h) * 2 * CR_MAX_CLASSES * sizeof(unsigned long long); }

#define HIPCHK(h, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
            return DEMCZ_ERR_HIP;                                                                \
        }                                                                                        \
    } while (0)

#define NCCLCHK(h, expr)                                                                         \
    do {                                                                                         \
        ncclResult_t r_ = (expr);                                                                \
        if (r_ != ncclSuccess) {                                                                 \
            (h)->err = std::string(#expr) + ": " + ncclGetErrorString(r_);                       \
            return DEMCZ_ERR_COMM;                                                               \
        }                                                                                        \
    } while (0)


#define DEADCHK(h)                                                                               \
    do {                                                                                         \
        if ((h)->comm_dead) return DEMCZ_ERR_COMM;                                               \
    } while (0)

static int32_t fail(demcz_handle* h, int32_t code, const std::string& msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

static int32_t refuse_derived(const demcz_handle* h, const char* who)
{
    if (!h || !h->derived) return DEMCZ_OK;
    return fail(const_cast<demcz_handle*>(h), DEMCZ_ERR_STATE,
                std::string(who) + ": the handle is a derived history (demcz_derive): it takes the statistics over its values, demcz_get_history "
                                   "without log_obj, demcz_derive, demcz_pointwise, demcz_loo, demcz_bridge_iterate, demcz_synchronize and demcz_destroy, and nothing else");
}
// first statement of every entry point a derived history does not take (a NULL handle is left to the function's own check)
#define NOT_DERIVED(h)                                                                           \
    do {                                                                                         \
        int32_t rd_ = refuse_derived((h), __func__);                                             \
        if (rd_) return rd_;                                                                     \
    } while (0)

// ---- comm failure path ---------------------------------------------------------------------------------------------
// A sharded handle's streams carry RCCL kernels that wait for PEERS: a dead or wedged peer would make every blocking
// wait on such a stream (or on an event behind one) wait for ever, on every rank -- the worst failure mode on a shared
// pool.  So a sharded handle never blocks in the runtime: it polls (hipStreamQuery / hipEventQuery), looks at
// ncclCommGetAsyncError of both communicators about once a millisecond, and gives up at the deadline
// (demcz_set_comm_timeout, default 60 s; DEMCZ_COMM_TIMEOUT_MS): ncclCommAbort on both communicators (their kernels
// leave, the streams drain), the handle is marked dead and DEMCZ_ERR_COMM is returned from this and every later call.
// A fresh process is the only retry.  Unsharded handles wait in the runtime as before.
namespace demcz {
__global__ void mark_kernel(volatile long long* word, long long value)
{
    __hip_atomic_store(const_cast<long long*>(word), value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Are the kernels of R streams able to run at the same time?  Each adds one to a counter and waits (bounded) until all R have.
__global__ void rendezvous_kernel(unsigned int* ctr, unsigned int R, unsigned int* met, unsigned long long max_ticks)
{
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = wall_clock64();           // 100 MHz
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < R && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(16);
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= R) __hip_atomic_fetch_add(met, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// First contact between the replicas of a sharded run (demcz_comm_init): every rank stores a token into slot `rank` of every
// peer's mailbox -- the same write-through, system-scope 8-byte store live_publish uses for a row, through the same IPC mapping,
// into the same fine-grained allocation (the mailbox is its last 4 KiB) -- and polls its OWN mailbox, at system scope like
// live_reload, until all R tokens are there or the time is up.  What the in-launch hand-off rests on -- a store from another
// GPU's running kernel becoming visible to a polling kernel here -- is thereby checked on the real links before any row
// depends on it; result[0] = 1 if all tokens arrived, result[1] = 100 MHz ticks this rank waited for the last of them.
struct PingBoxes { unsigned long long* box[DEMCZ_MAX_PEERS]; };
__global__ void peer_ping_kernel(unsigned long long* own, PingBoxes peers, int n_peers, int rank, int R, unsigned long long token,
                                 unsigned long long max_ticks, unsigned int* result)
{
    const int lane = (int)threadIdx.x;
    if (lane < n_peers) __hip_atomic_store(peers.box[lane] + rank, token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (lane == 0) __hip_atomic_store(own + rank, token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long t0 = wall_clock64();
    bool ok = lane >= R;
    while (!ok && wall_clock64() - t0 < max_ticks) {
        ok = __hip_atomic_load(own + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == token;
        if (!ok) __builtin_amdgcn_s_sleep(8);
    }
    const unsigned long long waited = wall_clock64() - t0;
    const bool all = __builtin_amdgcn_ballot_w64(ok) == __builtin_amdgcn_ballot_w64(true);
    unsigned long long wmax = waited;
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(wmax, o, 64); wmax = v > wmax ? v : wmax; }
    if (lane == 0) { result[0] = all ? 1u : 0u; result[1] = (unsigned int)(wmax > 0xffffffffull ? 0xffffffffull : wmax); }
}
__global__ void stall_kernel(int* release, unsigned long long max_ticks)
{
    const unsigned long long t0 = wall_clock64();           // 100 MHz
    while (__hip_atomic_load(release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(32);
}
}  // namespace demcz

static int32_t comm_fail(demcz_handle* h, const std::string& why)
{
    h->comm_dead = true;
    if (h->stall_flag) {                                      // (a test's stall kernel leaves at once: a device word, set from a stream of its own)
        hipStream_t rs = nullptr;
        if (hipStreamCreateWithFlags(&rs, hipStreamNonBlocking) == hipSuccess) {
            (void)hipMemsetAsync(h->stall_flag, 0xff, sizeof(int), rs);
            (void)hipStreamSynchronize(rs);
            (void)hipStreamDestroy(rs);
        }
    }
    if (h->comm_side) (void)ncclCommAbort(h->comm_side);
    if (h->comm) (void)ncclCommAbort(h->comm);
    h->comm_side = nullptr;                                   // (abort frees them; `comm` stays non-null as the "sharded" mark
    // bounded drain: with the collectives gone the streams should run dry; do not wait for ever for that either
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t ss[5] = {h->stream, h->comm_stream, h->prod_stream, h->diag_stream, h->hs_stream};
    for (hipStream_t st : ss) {
        if (!st) continue;
        while (hipStreamQuery(st) == hipErrorNotReady &&
               std::chrono::steady_clock::now() - t0 < std::chrono::seconds(1)) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    h->err = "communication failure (" + why + "): both RCCL communicators aborted; the handle is dead -- restart the job in fresh processes";
    return DEMCZ_ERR_COMM;
}

template <class Query>
static int32_t wait_deadline(demcz_handle* h, Query query, const char* what)
{
    static const bool dbg = getenv("DEMCZ_DEBUG_COMM") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto last_check = t0;
    for (unsigned long long polls = 0;; ++polls) {
        const hipError_t e = query();
        if (e == hipSuccess) {
            if (dbg) fprintf(stderr, "[demcz] wait %s: done after %llu polls, %.3f ms\n", what, polls,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            return DEMCZ_OK;
        }
        if (e != hipErrorNotReady) { h->err = std::string(what) + ": " + hipGetErrorString(e); return DEMCZ_ERR_HIP; }
        const auto now = std::chrono::steady_clock::now();
        if (now - last_check >= std::chrono::milliseconds(1)) {
            last_check = now;
            for (ncclComm_t c : {h->comm, h->comm_side}) {
                if (!c) continue;
                ncclResult_t ar = ncclSuccess;
                const ncclResult_t qr = ncclCommGetAsyncError(c, &ar);
                if (qr != ncclSuccess || (ar != ncclSuccess && ar != ncclInProgress))
                    return comm_fail(h, std::string(what) + ": RCCL reports " + ncclGetErrorString(qr != ncclSuccess ? qr : ar));
            }
            if (h->comm_timeout_ms > 0 && now - t0 >= std::chrono::milliseconds(h->comm_timeout_ms))
                return comm_fail(h, std::string(what) + ": no progress within " + std::to_string(h->comm_timeout_ms) + " ms -- a peer rank is dead or stalled");
        }
        if (polls > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));      // (spin first: most waits are short)
    }
}

static int32_t sync_stream(demcz_handle* h, hipStream_t s, const char* what)
{
    if (h->comm_dead) return DEMCZ_ERR_COMM;
    if (!h->comm) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { h->err = std::string(what) + ": hipStreamSynchronize: " + hipGetErrorString(e); return DEMCZ_ERR_HIP; }
        return DEMCZ_OK;
    }
    return wait_deadline(h, [s]() { return hipStreamQuery(s); }, what);
}

static int32_t sync_event(demcz_handle* h, hipEvent_t ev, const char* what)
{
    if (h->comm_dead) return DEMCZ_ERR_COMM;
    if (!h->comm) {
        const hipError_t e = hipEventSynchronize(ev);
        if (e != hipSuccess) { h->err = std::string(what) + ": hipEventSynchronize: " + hipGetErrorString(e); return DEMCZ_ERR_HIP; }
        return DEMCZ_OK;
    }
    return wait_deadline(h, [ev]() { return hipEventQuery(ev); }, what);
}

#define SYNCCHK_AS(h, s, who)                                                                    \
    do {                                                                                         \
        int32_t rcs_ = sync_stream((h), (s), (who));                                             \
        if (rcs_) return rcs_;                                                                   \
    } while (0)
#define SYNCCHK(h, s) SYNCCHK_AS(h, s, __func__)

// hipFree / hipMalloc synchronise the whole device: before either, every stream of a sharded handle is waited for HERE, with
// the deadline -- so that a stalled peer surfaces as DEMCZ_ERR_COMM instead of a runtime call that never returns.
static int32_t quiesce_all(demcz_handle* h)
{
    if (h->comm_dead) return DEMCZ_ERR_COMM;
    if (!h->comm) return DEMCZ_OK;
    for (hipStream_t st : {h->stream, h->comm_stream, h->prod_stream, h->diag_stream, h->hs_stream})
        if (st) { int32_t rc = sync_stream(h, st, "quiesce"); if (rc) return rc; }
    return DEMCZ_OK;
}

// test hook (demcz_debug_stall_exchange): a kernel that holds the stream the next collective goes to
static int32_t maybe_stall(demcz_handle* h, hipStream_t s)
{
    if (h->stall_next_ms <= 0) return DEMCZ_OK;
    if (getenv("DEMCZ_DEBUG_COMM")) fprintf(stderr, "[demcz] stall kernel of %d ms enqueued\n", h->stall_next_ms);
    if (!h->stall_flag) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->stall_flag, sizeof(int)));
    HIPCHK(h, hipMemsetAsync(h->stall_flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(1), 0, s, h->stall_flag, (unsigned long long)h->stall_next_ms * 100000ull);
    HIPCHK(h, hipGetLastError());
    h->stall_next_ms = 0;
    return DEMCZ_OK;
}

static int64_t blockstep_nblk(int b)
{
    const int nn = (b == 1) ? 1 : b;
    return 1 + (nn + 1) / 2 + 1;
}

constexpr size_t ML_MAX_DYNAMIC_LDS = 160 * 1024;      // LDS per CU on gfx950
constexpr size_t PEER_MAILBOX_BYTES = 4096;            // behind a fine-grained archive: peer_ping_kernel's tokens
constexpr size_t REC_PAD = 64;       // doubles behind a record buffer: a consumer's fetches may run past its last row's last generation
constexpr int PC_CONSUMER_CHAINS = 8;       // chains per consumer workgroup of the replicated split layout: 8 lanes per chain
static int ml_lanes_available(int target_kind, int d, bool full_block, int64_t nobs, int max_blocklen, int nblocks);
static bool pc_available(int target_kind, int d, bool full_block);
static bool mlb32_wanted(int64_t N);
static bool split_ml_available(int target_kind, int d, bool full_block, int64_t nobs);
static bool ps_available(int target_kind, int d);
static int64_t live_wg_capacity(demcz_handle* h);
static WindowKernel window_kernel_of(const demcz_handle* h, const LaunchFacts& f);
static LaunchFacts launch_facts(const demcz_handle* h, const WindowParams* P, bool live);
constexpr int MAX_LIVE_KERNELS = 6;
static int live_kernels(const demcz_handle* h, WindowKernel out[MAX_LIVE_KERNELS]);
// the draw records on the device no longer match what the next launch will need (or are about to be freed): nothing of
// the side-stream producer may still be writing them
static void rec_invalidate(demcz_handle* h)
{
    if (h->prod_stream) (void)hipStreamSynchronize(h->prod_stream);
    h->prod_pending[0] = h->prod_pending[1] = false;
    h->rec_desc[0].valid = h->rec_desc[1].valid = false;
}
// The archive is about to get SHORTER (a rollback, a new demcz_set_state, a discarded speculative slab): the record buffers may hold
// row indices drawn against the longer one.  No launch consumes them -- rec_invalidate makes the next launch draw its own -- but
// the wave-per-chain kernels prefetch a pass or two past a launch's last generation, out of whatever the buffer holds there,
// and a prefetched index of an unwritten row reads the sentinel.  Zeros ("row 0: always a legal index") again, as at allocation.
static int32_t rec_scrub(demcz_handle* h)
{
    rec_invalidate(h);
    if (h->lanes != DEMCZ_LAYOUT_SPLIT || h->rec_cap <= 0 || getenv("DEMCZ_NO_SCRUB")) return DEMCZ_OK;
    for (int b = 0; b < 2; ++b) {
        if (!h->d_rec[b]) continue;
        const size_t per = h->rec_in_arena ? (size_t)(h->cfg.d + 2) : (size_t)((h->split_kind == SPLIT_MLB) ? 2 * h->S : (int64_t)h->cfg.d + 2);
        const size_t nd = (size_t)h->rec_cap * per * (size_t)h->cfg.N + REC_PAD;
        HIPCHK(h, hipMemsetAsync(h->d_rec[b], 0, nd * sizeof(double), h->stream));
    }
    return DEMCZ_OK;
}
static int32_t flush_exchanges(demcz_handle* h);
static void peer_detach(demcz_handle* h);
static void peer_no_dual(demcz_handle* h);
static int32_t peer_setup_ipc(demcz_handle* h);
static bool peer_capable(const demcz_handle* h);
static int32_t check_live_err(demcz_handle* h);
static int32_t live_verify(demcz_handle* h);
static int32_t group_verify(demcz_handle* h);
static int32_t live_failed(demcz_handle* h, bool& failed);
static void live_release(demcz_handle* h);
static int64_t live_span(demcz_handle* h);
static int64_t rec_target_bytes(bool dual);
static int32_t rec_reserve(demcz_handle* h, int64_t gens);
static int32_t check_hist_range(demcz_handle* h, int64_t g_from, int64_t g_to, const char* who);
static bool ps2_applicable(const demcz_handle* h, const WindowParams& P);

extern "C" int32_t demcz_abi_version(void) { return DEMCZ_ABI_VERSION; }

extern "C" const char* demcz_last_error(const demcz_handle* h)
{
    return h ? h->err.c_str() : g_create_error.c_str();
}

template <class T>
static hipError_t dev_alloc_copy(T** dst, const T* src, size_t n, hipStream_t s, int device)
{
    hipError_t e = dev_malloc(device, (void**)dst, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, s);
    return e;
}

static void free_all(demcz_handle* h)
{
    // Buffers only go back to the pools when nothing can still be touching them: every stream of the handle has run dry
    // (demcz_destroy waits for them) and no communicator was aborted under it.  Otherwise they are freed -- hipFree / hipHostFree
    // wait for the device, which is what the pools exist to avoid but is the only safe thing then.
    bool drained = !h->comm_dead;
    for (hipStream_t st : {h->stream, h->prod_stream, h->diag_stream, h->comm_stream, h->hs_stream})
        if (st && hipStreamQuery(st) != hipSuccess) drained = false;
    if (h->d_acc) (void)dev_free(h->cfg.device_id, h->d_acc);
    if (h->d_cr_counts) (void)dev_free(h->cfg.device_id, h->d_cr_counts);
    if (h->d_cr_adapt) (void)dev_free(h->cfg.device_id, h->d_cr_adapt);
    if (h->d_err_all) (void)dev_free(h->cfg.device_id, h->d_err_all);
    if (h->archive_fine) { if (h->dZ) (void)hipFree(h->dZ); h->dZ = nullptr; }     // (an allocation of its own: demcz_comm_init)
    if (h->pooled_dev) {               // (the two big ones)
        if (h->archive_fine) {
        } else if (drained) {
            g_dev_pool.release(h->dZ, h->cfg.device_id);
        } else {
            g_dev_pool.discard(h->dZ);
        }
        if (h->hist_joint) { if (drained) g_dev_pool.release(h->dchain_alloc, h->cfg.device_id); else g_dev_pool.discard(h->dchain_alloc); }
        h->dZ = nullptr;
        if (h->hist_joint) { h->dchain = nullptr; h->dchain_alloc = nullptr; }
    }
    if (h->hs_stream) stream_release(h->cfg.device_id, h->hs_stream, drained);
    if (drained) { g_host_pool.release(h->hs_chain, -1); g_host_pool.release(h->hs_logobj, -1); }
    else { g_host_pool.discard(h->hs_chain); g_host_pool.discard(h->hs_logobj); }
    void* bufs[] = {h->dZ, h->dX, h->dlp, h->dchain, h->hist_joint ? nullptr : h->dlogobj, h->dlp_origin, h->dtemp, h->d_block_offsets,
                    h->d_slot_of, h->d_slot_role, h->d_eps, h->d_mu, h->d_Wp, h->d_design, h->d_y, h->d_scratch, h->dXprop,
                    h->dlogu, h->d_gather};
    for (void* b : bufs)
        if (b) (void)dev_free(h->cfg.device_id, b);
    for (auto& pe : h->pending) if (pe.ev) (void)hipEventDestroy(pe.ev);
    h->pending.clear();
    for (int b = 0; b < 2; ++b) {
        if (h->d_rec[b] && !h->rec_in_arena) (void)dev_free(h->cfg.device_id, h->d_rec[b]);
        if (b == 0 && h->d_live_err) (void)dev_free(h->cfg.device_id, h->d_live_err);
        if (h->d_send[b]) (void)dev_free(h->cfg.device_id, h->d_send[b]);
        if (h->d_recv[b]) (void)dev_free(h->cfg.device_id, h->d_recv[b]);
        if (h->buf_done[b]) (void)hipEventDestroy(h->buf_done[b]);
    }
    if (h->comm_stream) stream_release(h->cfg.device_id, h->comm_stream, !h->comm_dead && hipStreamQuery(h->comm_stream) == hipSuccess);
    if (h->prod_stream) { if (!h->comm_dead) (void)hipStreamSynchronize(h->prod_stream); stream_release(h->cfg.device_id, h->prod_stream, !h->comm_dead); }
    for (int b = 0; b < 2; ++b) if (h->prod_done[b]) (void)hipEventDestroy(h->prod_done[b]);
    if (h->prod_gate) (void)hipEventDestroy(h->prod_gate);
    if (h->d_stage) (void)host_free(h->d_stage);
    for (auto& pr : h->timed) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (h->pinned_rhat) (void)host_free(h->pinned_rhat);
    if (h->pinned_err) (void)host_free(h->pinned_err);
    if (h->d_safe_X) (void)dev_free(h->cfg.device_id, h->d_safe_X);
    if (h->d_safe_lp) (void)dev_free(h->cfg.device_id, h->d_safe_lp);
    if (h->d_spec_X) (void)dev_free(h->cfg.device_id, h->d_spec_X);
    if (h->d_spec_lp) (void)dev_free(h->cfg.device_id, h->d_spec_lp);
    if (h->spec_ev) (void)hipEventDestroy(h->spec_ev);
    if (h->diag_ev) (void)hipEventDestroy(h->diag_ev);
    if (h->rhat_side_ev) (void)hipEventDestroy(h->rhat_side_ev);
    if (h->diag_stream) stream_release(h->cfg.device_id, h->diag_stream, !h->comm_dead && hipStreamQuery(h->diag_stream) == hipSuccess);
    if (h->stall_flag) (void)dev_free(h->cfg.device_id, h->stall_flag);
    if (h->hc_X) (void)hipHostFree(h->hc_X);
    if (h->hc_lp) (void)hipHostFree(h->hc_lp);
    if (h->hc_flag) (void)hipHostFree(const_cast<unsigned int*>(h->hc_flag));
    if (h->hc_count) (void)dev_free(h->cfg.device_id, h->hc_count);
    if (h->xdone) (void)host_free(const_cast<long long*>(h->xdone));
    if (!h->comm_dead) {                 // (a dead handle's communicators were aborted, which frees them)
        if (h->comm_side) (void)ncclCommDestroy(h->comm_side);
        if (h->comm) (void)ncclCommDestroy(h->comm);
    }
    if (h->own_stream && h->stream) stream_release(h->cfg.device_id, h->stream, !h->comm_dead && hipStreamQuery(h->stream) == hipSuccess);
}

extern "C" int32_t demcz_create(demcz_handle** out, const demcz_config* cfg)
{
    if (!out || !cfg) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: null argument");
    *out = nullptr;
    if (cfg->N < 1 || cfg->d < 1 || cfg->d > MAX_D || cfg->K < 1 || cfg->Mcap < 2 || cfg->Gcap < 0 ||
        cfg->Nblocks < 1 || !cfg->block_offsets || !cfg->block_indices || !cfg->eps_scale || cfg->chain_id0 < 0)
        return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT,
                    "demcz_create: need N>=1, 1<=d<=64, K>=1, Mcap>=2, Gcap>=0, Nblocks>=1 and block/eps tables");
    if (cfg->lanes_per_chain != 0 && cfg->lanes_per_chain != 1 && cfg->lanes_per_chain != 8 && cfg->lanes_per_chain != 16 &&
        cfg->lanes_per_chain != DEMCZ_LAYOUT_SPLIT && cfg->lanes_per_chain != DEMCZ_LAYOUT_SPLIT_WAVE &&
        cfg->lanes_per_chain != DEMCZ_LAYOUT_PROGRAM_WAVE)
        return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT,
                    "demcz_create: lanes_per_chain must be 0 (auto), 1, 8, 16, DEMCZ_LAYOUT_SPLIT, DEMCZ_LAYOUT_SPLIT_WAVE or (program targets) "
                    "DEMCZ_LAYOUT_PROGRAM_WAVE");
    if (cfg->lanes_per_chain == DEMCZ_LAYOUT_PROGRAM_WAVE && cfg->target_kind != DEMCZ_TARGET_PROGRAM)
        return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: DEMCZ_LAYOUT_PROGRAM_WAVE is the wave-per-chain layout of program targets: "
                                                         "target_kind must be DEMCZ_TARGET_PROGRAM (built-in targets: DEMCZ_LAYOUT_SPLIT_WAVE)");
    const int d = cfg->d;
    // validate blocks: offsets ascending, indices within range and unique inside a block
    if (cfg->block_offsets[0] != 0) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "block_offsets[0] must be 0");
    for (int ib = 0; ib < cfg->Nblocks; ++ib) {
        const int a = cfg->block_offsets[ib], b = cfg->block_offsets[ib + 1];
        if (b <= a || b - a > d) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "empty or oversized block");
        for (int t = a; t < b; ++t) {
            if (cfg->block_indices[t] < 0 || cfg->block_indices[t] >= d)
                return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "block index out of range");
            for (int u = a; u < t; ++u)
                if (cfg->block_indices[u] == cfg->block_indices[t])
                    return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "duplicate index inside a block");
        }
    }
    switch (cfg->target_kind) {
    case DEMCZ_TARGET_MVNORMAL:
        if (!cfg->mu || !cfg->W) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "MVNORMAL needs mu and W");
        break;
    case DEMCZ_TARGET_ISO_QUAD:
        if (!cfg->mu) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "ISO_QUAD needs mu");
        break;
    case DEMCZ_TARGET_LINREG_SSE:
        if (!cfg->design || !cfg->yobs || cfg->nobs < 1)
            return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "LINREG_SSE needs design, yobs, nobs>=1");
        break;
    case DEMCZ_TARGET_HOST_CALLBACK: break;
    case DEMCZ_TARGET_PROGRAM:
        // (the program is compiled into the one-lane window kernel or, on request, into the wave-per-chain consumer -- one whole
        //  candidate per lane; the cooperating-lane layouts split the log-density across lanes, which a user's scalar function
        //  cannot be)
        if (cfg->lanes_per_chain != 0 && cfg->lanes_per_chain != 1 && cfg->lanes_per_chain != DEMCZ_LAYOUT_PROGRAM_WAVE)
            return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: a program target runs one lane per chain: lanes_per_chain must be 0 or 1 "
                                                             "(or DEMCZ_LAYOUT_PROGRAM_WAVE: one wavefront per chain)");
        if (cfg->d > demcz_prog::MAX_PROGRAM_D)
            return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: a program target needs 1 <= d <= 32");
        if (cfg->lanes_per_chain == DEMCZ_LAYOUT_PROGRAM_WAVE) {
            bool one_block = cfg->Nblocks == 1 && cfg->block_offsets[1] == d;
            for (int p = 0; one_block && p < d; ++p) one_block = cfg->block_indices[p] == p;
            if (!one_block)
                return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: DEMCZ_LAYOUT_PROGRAM_WAVE needs one block 0..d-1 in order (block updates run one lane per chain)");
            if (d < demcz_prog::WAVE_MIN_D)
                return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: DEMCZ_LAYOUT_PROGRAM_WAVE needs 2 <= d <= 32");
            if (cfg->N > PS_MAX_N)
                return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: DEMCZ_LAYOUT_PROGRAM_WAVE needs N <= " + std::to_string(PS_MAX_N) +
                                                                 " (one wavefront per chain: PS_MAX_N)");
            if (!(cfg->Mcap <= 0xffffffffll && (double)cfg->Mcap * 8.0 * (((d + 7) / 8) * 8) < 4294967296.0))
                return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: DEMCZ_LAYOUT_PROGRAM_WAVE needs an archive reachable by 32-bit offsets: "
                                                                 "Mcap * 8 * (d rounded up to a multiple of 8) < 2^32");
        }
        break;
    default: return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "unknown target_kind");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, DEMCZ_ERR_NO_DEVICE, "demcz_create: no HIP device visible (there is no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_create: device_id out of range");

    demcz_handle* h = new demcz_handle();
    h->cfg = *cfg;
    h->lanes = 1;
    if (const char* re = getenv("DEMCZ_LIVE_REARMS")) h->live_rearms_left = std::max(0, atoi(re));
    auto bail = [&](int32_t code) {
        g_create_error = h->err;
        free_all(h);
        delete h;
        return code;
    };
#define CRCHK(expr)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
            return bail(DEMCZ_ERR_HIP);                                                          \
        }                                                                                        \
    } while (0)
    CRCHK(hipSetDevice(cfg->device_id));
    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
    } else {
        CRCHK(stream_acquire(cfg->device_id, &h->stream));
        h->own_stream = true;
    }
    h->block_offsets.assign(cfg->block_offsets, cfg->block_offsets + cfg->Nblocks + 1);
    h->block_indices.assign(cfg->block_indices, cfg->block_indices + h->block_offsets.back());
    h->eps.assign(cfg->eps_scale, cfg->eps_scale + d);
    h->slot_of.assign((size_t)cfg->Nblocks * d, -1);
    h->S = 0;
    for (int ib = 0; ib < cfg->Nblocks; ++ib) {
        const int a = h->block_offsets[ib], b = h->block_offsets[ib + 1];
        for (int t = a; t < b; ++t) h->slot_of[(size_t)ib * d + h->block_indices[t]] = t - a;
        h->S += blockstep_nblk(b - a);
    }
    h->S_plain = h->S;
    h->full_block = (cfg->Nblocks == 1 && h->block_offsets[1] == d);
    if (h->full_block)
        for (int p = 0; p < d; ++p) h->full_block = h->full_block && (h->block_indices[p] == p);
    if (cfg->target_kind == DEMCZ_TARGET_MVNORMAL && cfg->Nblocks >= 2 && h->block_offsets.back() == d) {
        // the blocks, in order, are consecutive index ranges covering 0..d-1 (any order of the indices inside a block): the sums
        // of the quadratic form are cut at their boundaries (the grouped order)
        bool ok = true;
        uint64_t starts = 0;
        for (int ib = 0; ib < cfg->Nblocks && ok; ++ib) {
            const int lo = h->block_offsets[ib], hi = h->block_offsets[ib + 1];
            uint64_t seen = 0;
            for (int t = lo; t < hi; ++t) {
                const int j = h->block_indices[t];
                if (j < lo || j >= hi || ((seen >> (j - lo)) & 1ull)) { ok = false; break; }
                seen |= 1ull << (j - lo);
            }
            starts |= 1ull << lo;
        }
        if (ok) {
            h->ngrp = cfg->Nblocks;
            h->gstart = starts;
            bool equal = true;
            for (int ib = 0; ib < cfg->Nblocks; ++ib) equal = equal && (h->block_offsets[ib + 1] - h->block_offsets[ib] == h->block_offsets[1]);
            if (equal && d == 20 && h->block_offsets[1] == 5 && !getenv("DEMCZ_NO_MLB_INCREMENTAL")) h->mlb_qb = 5;      // C3: 4 x 5
        }
    }
    {   // layout: L lanes per chain when the chip would otherwise sit idle (small N), else one lane
        int maxb = 0;
        for (int ib = 0; ib < cfg->Nblocks; ++ib) maxb = std::max(maxb, h->block_offsets[ib + 1] - h->block_offsets[ib]);
        const int L = ml_lanes_available(cfg->target_kind, d, h->full_block, cfg->nobs, maxb, cfg->Nblocks);
        // d = 20 in blocks, split form chosen by the library: 32 lanes per chain (two chains to a wave, one parameter a lane)
        const int Lsplit = (L == 16 && d == 20 && !h->full_block && cfg->lanes_per_chain == 0 && cfg->N <= 4096 && mlb32_wanted(cfg->N)) ? 32 : L;
        // 32-bit row indices in the records, 32-bit byte offsets into the archive
        const bool idx32 = cfg->Mcap <= 0xffffffffll && (double)cfg->Mcap * 8.0 * (((d + 7) / 8) * 8) < 4294967296.0;
        const SplitKind kind = !idx32 ? SPLIT_NONE : pc_available(cfg->target_kind, d, h->full_block) ? SPLIT_PC8
                               : split_ml_available(cfg->target_kind, d, h->full_block, cfg->nobs) ? SPLIT_ML
                               : (!h->full_block && cfg->target_kind == DEMCZ_TARGET_MVNORMAL && L > 1) ? SPLIT_MLB : SPLIT_NONE;
        h->split_lanes = (kind == SPLIT_ML) ? 16 : (kind == SPLIT_MLB) ? Lsplit : 0;
        {   // four-wave workgroups once there is a chain wave for every SIMD (see demcz_kernels_ml.h, ML_WAVES)
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id) != hipSuccess) cus = 0;
            const int lanes_pc = (kind == SPLIT_ML) ? 16 : (kind == SPLIT_MLB) ? Lsplit : (L > 1 ? L : 64);
            const int64_t chain_waves = (cfg->N * lanes_pc + 63) / 64;
            h->wpw = (cus > 0 && chain_waves >= 4ll * cus) ? ML_WAVES : 1;
        }
        // chains per consumer workgroup
        h->split_per_wg = (kind == SPLIT_PC8) ? PC_CONSUMER_CHAINS : (kind == SPLIT_ML) ? ((cfg->target_kind == DEMCZ_TARGET_LINREG_SSE) ? LR16_CHAINS : 4 * h->wpw)
                          : (kind == SPLIT_MLB) ? h->wpw * (64 / Lsplit) : 1;
        const bool split_ok = kind != SPLIT_NONE;
        // one wave per chain (demcz_kernels_ps.h): where the replicated consumer is built and a pass's draws fit one DMA
        // (round 5: wherever the archive's rows are reachable by 32-bit offsets -- no longer only where another split consumer is
        //  built for the dimension too)
        const bool ps_ok = idx32 && h->full_block && ps_available(cfg->target_kind, d);
        const int per_wg_default = h->split_per_wg;
        h->split_kind = SPLIT_NONE;
        if (cfg->lanes_per_chain == DEMCZ_LAYOUT_PROGRAM_WAVE) {
            // (validated above.  How many chains a LIVE launch holds depends on the program's registers and is known once
            //  demcz_set_program has compiled it: live_wg_capacity.  More than that, up to PS_MAX_N: one launch per K-window.)
            h->prog_wave = true;
            h->lanes = DEMCZ_LAYOUT_SPLIT;
            h->split_kind = SPLIT_WAVE;
            h->split_per_wg = PS_CHAINS;
            h->split_lanes = 0;
        } else
        if (cfg->lanes_per_chain == DEMCZ_LAYOUT_SPLIT_WAVE || (cfg->lanes_per_chain == 0 && ps_ok && cfg->N <= PS_MAX_N && cfg->K >= 2 && !getenv("DEMCZ_NO_PS"))) {
            // (us per K-window at d=5, one wave per chain / eight replicated lanes: see DESIGN.md, K1g; K = 1 leaves a
            //  pass one generation: 1.05 against 0.99 us per generation, scripts/k_small.py)
            if (!ps_ok) {
                h->err = "demcz_create: the wave-per-chain split layout is not built for this target / d / block structure";
                return bail(DEMCZ_ERR_INVALID_ARGUMENT);
            }
            h->lanes = DEMCZ_LAYOUT_SPLIT;
            h->split_kind = SPLIT_WAVE;
            h->split_per_wg = PS_CHAINS;
            // The library's own choice also asks that the consumers of a LIVE launch all fit the chip at once (one launch
            // per K-window is where this layout loses to the replicated consumer): MI355X, d = 5: 1024 chains.
            // Two chains to a wave (window_kernel_ps2d, d <= 5, K a multiple of five): where one chain per wave no longer fits a LIVE
            // launch (N > 1024 on MI355X) but half as many waves do -- up to 2048 chains.  DEMCZ_PS_DUAL=1 forces it at any N (tests).
            const bool dual_env = getenv("DEMCZ_PS_DUAL") != nullptr && atoi(getenv("DEMCZ_PS_DUAL")) != 0;
            const bool dual_ok = d >= 2 && d <= 5 && cfg->K % 5 == 0 && !getenv("DEMCZ_NO_PS2") && !getenv("DEMCZ_NO_PS_DUAL");
            const bool single_fits = (cfg->N + PS_CHAINS - 1) / PS_CHAINS <= live_wg_capacity(h);
            if (dual_ok && (dual_env || (!single_fits && cfg->lanes_per_chain == 0))) {
                h->ps_dual = true;
                h->split_per_wg = 2 * PS_CHAINS;
                h->live_wg_cap = -1;
                if (!dual_env && (cfg->N + 2 * PS_CHAINS - 1) / (2 * PS_CHAINS) > live_wg_capacity(h)) {      // not even that fits
                    h->ps_dual = false;
                    h->split_per_wg = PS_CHAINS;
                    h->live_wg_cap = -1;
                }
            }
            if (!h->ps_dual && cfg->lanes_per_chain == 0 && !single_fits && kind != SPLIT_NONE) {
                h->split_kind = kind;
                h->split_per_wg = per_wg_default;
                h->live_wg_cap = -1;
            }
            // (kind == SPLIT_NONE -- a dimension with no other split consumer -- and more chains than a LIVE launch holds, up to PS_MAX_N:
            //  one wave per chain all the same, one launch per K-window; the alternative is the one-lane kernel's 16-32 waves)
        } else if (cfg->lanes_per_chain == DEMCZ_LAYOUT_SPLIT) {
            if (!split_ok) {
                h->err = "demcz_create: the split layout is not built for this target / d / block structure";
                return bail(DEMCZ_ERR_INVALID_ARGUMENT);
            }
            h->lanes = DEMCZ_LAYOUT_SPLIT;
            h->split_kind = kind;
        } else if (cfg->lanes_per_chain == 0 && split_ok && cfg->N <= (kind == SPLIT_PC8 ? 8192 : 4096)) {
            // (16 cooperating lanes, d = 20, us per K-window split / fused: N=1024 9.7 / 16.8, N=4096 16.6 / 21.0,
            //  N=8192 35.5 / 29.8)
            h->split_kind = kind;
            // idle CUs do the state-independent three quarters of the work.  Measured at d=5, us per
            // K-window, split / 8 lanes per chain / 1 lane: N=4096 8.6 / 12.4 / 30.0, N=16384 22.4 / 19.0 /
            // 32.6, N=32768 41.4 / 29.7 / 35.7, N=65536 77.7 / 54.5 / 40.9
            h->lanes = DEMCZ_LAYOUT_SPLIT;
        } else if (cfg->lanes_per_chain > 1) {
            if (L != cfg->lanes_per_chain) {
                h->err = "demcz_create: the requested lanes_per_chain layout is not built for this target / d / block structure";
                return bail(DEMCZ_ERR_INVALID_ARGUMENT);
            }
            h->lanes = L;
        } else if (cfg->lanes_per_chain == 0 && L > 1 && cfg->N * L <= 262144) {
            h->lanes = L;       // up to ~4 waves per SIMD; measured crossover with one lane per chain at d=5:
        }                       // N=32768 29.9 vs 35.4 us per window, N=65536 53.8 vs 45.8
    }
    if (h->lanes == DEMCZ_LAYOUT_SPLIT && h->split_kind == SPLIT_ML && cfg->target_kind == DEMCZ_TARGET_LINREG_SSE && !getenv("DEMCZ_NO_LR_SPEC")) {
        // Eight chains per workgroup, two generations per log-density pass, where that still is at most one workgroup per CU
        // (C5: 2048 chains = 256 workgroups; sixteen chains per workgroup leave half the chip idle there).
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id) != hipSuccess) cus = 0;
        if ((cfg->N + LR8_CHAINS - 1) / LR8_CHAINS <= (int64_t)cus && lr8s_dynamic_lds<10>(cfg->nobs) <= ML_MAX_DYNAMIC_LDS) {
            h->lr_spec = true;
            h->split_per_wg = LR8_CHAINS;
        }
    }
    // no pointer of the caller's survives create
    h->cfg.block_offsets = nullptr; h->cfg.block_indices = nullptr; h->cfg.eps_scale = nullptr;
    h->cfg.mu = nullptr; h->cfg.W = nullptr; h->cfg.design = nullptr; h->cfg.yobs = nullptr; h->cfg.stream = nullptr;
    if (cfg->target_kind == DEMCZ_TARGET_PROGRAM) h->cfg.nobs = 0;      // (ndata, once demcz_set_program has run)

    const int64_t N = cfg->N;
    const int64_t N_for_arena = cfg->N;
    h->ZS = (d <= 1) ? 2 : (d <= 2) ? 2 : (d <= 4) ? 4 : ((d + 7) / 8) * 8;     // 16-byte aligned rows; d=5 -> one 64-byte line
    {
        size_t zbytes = (size_t)cfg->Mcap * h->ZS * sizeof(double);
        if (h->lanes == DEMCZ_LAYOUT_SPLIT && h->split_kind == SPLIT_WAVE && d <= 5 && !h->prog_wave && !getenv("DEMCZ_NO_PS2")) {
            // (record buffers as demcz_run would size them: a LIVE launch's span, bounded by the history window; a caller that
            //  outruns the arena gets separate buffers and the general kernel)
            // (demcz_slab_plan.h: 64 MiB of records per buffer -- 1170 generations at C2 --, twice the bytes for a two-chain handle,
            //  which has up to twice the chains; shorter buffers beside an archive that leaves less room below the 32-bit reach)
            const ArenaSpan as = arena_span(zbytes, N_for_arena, d, cfg->K, cfg->Gcap, rec_target_bytes(h->ps_dual), (int64_t)REC_PAD);
            const int64_t ag = as.gens;
            const size_t zb = as.zb, rb = as.rb, tb = as.tb;
            if (ag > 0 && zb + 2 * rb + tb < ARENA_LIMIT) {
                h->arena = true;
                h->arena_gens = ag;
                h->arena_span = as.span;
                CRCHK(g_dev_pool.acquire((void**)&h->dZ, zb + 2 * rb + tb, cfg->device_id));
                h->dZ_bytes = zb + 2 * rb + tb;
                unsigned char* base = reinterpret_cast<unsigned char*>(h->dZ);
                h->arena_rec[0] = reinterpret_cast<double*>(base + zb);
                h->arena_rec[1] = reinterpret_cast<double*>(base + zb + rb);
                h->arena_temp = reinterpret_cast<double*>(base + zb + 2 * rb);
                CRCHK(hipMemsetAsync(base + zb, 0, 2 * rb + tb, h->stream));       // row 0 / temperature 0: always legal
            }
        }
        if (!h->arena) { CRCHK(g_dev_pool.acquire((void**)&h->dZ, zbytes, cfg->device_id)); h->dZ_bytes = zbytes; }
        if (h->ps_dual && !h->arena) { h->ps_dual = false; h->split_per_wg = PS_CHAINS; h->live_wg_cap = -1; }      // (the two-chain kernel addresses the arena)
        h->pooled_dev = true;
    }
    // (the reference pads with zeros, demcz.jl:11; rows at or beyond M never leave the device, and here they hold
    //  the sentinel LIVE launches recognise an unpublished row by: fill_unwritten_rows() in demcz_set_state)
    CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->d_live_err, 4 * sizeof(unsigned int)));
    CRCHK(hipMemsetAsync(h->d_live_err, 0, 4 * sizeof(unsigned int), h->stream));
    CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->dX, (size_t)N * d * sizeof(double)));
    CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->dlp, (size_t)N * sizeof(double)));
    if (cfg->Gcap > 0) {
        // (one allocation: a window kernel's history store of a pass covers both arrays with one buffer descriptor)
        // (DEMCZ_DEBUG_HIST_SKEW=<bytes>: the history that many bytes into its allocation -- scripts/ps2_stamps.py, address classes)
        const size_t skew = getenv("DEMCZ_DEBUG_HIST_SKEW") ? ((size_t)atol(getenv("DEMCZ_DEBUG_HIST_SKEW")) & ~(size_t)7) : 0;
        CRCHK(g_dev_pool.acquire((void**)&h->dchain_alloc, (size_t)N * (d + 1) * cfg->Gcap * sizeof(double) + skew, cfg->device_id));
        h->dchain = h->dchain_alloc + skew / sizeof(double);
        h->dlogobj = h->dchain + (size_t)N * d * cfg->Gcap;
        h->hist_joint = true;
        CRCHK(hipMemsetAsync(h->dchain, 0, (size_t)N * (d + 1) * cfg->Gcap * sizeof(double), h->stream));   // demcz.jl:24
    }
    CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->dlp_origin, (size_t)N * sizeof(double)));
    CRCHK(dev_alloc_copy(&h->d_block_offsets, h->block_offsets.data(), h->block_offsets.size(), h->stream, cfg->device_id));
    CRCHK(dev_alloc_copy(&h->d_slot_of, h->slot_of.data(), h->slot_of.size(), h->stream, cfg->device_id));
    CRCHK(dev_alloc_copy(&h->d_eps, h->eps.data(), h->eps.size(), h->stream, cfg->device_id));
    {   // what every Philox block of a generation is: rows, a normal pair, or the accept uniform (per block, in order)
        std::vector<int32_t> role;
        for (int ib = 0; ib < cfg->Nblocks; ++ib) {
            const int nblk = (int)blockstep_nblk(h->block_offsets[ib + 1] - h->block_offsets[ib]);
            for (int t = 0; t < nblk; ++t) role.push_back(t == 0 ? 0 : (t == nblk - 1 ? 2 : 1));
        }
        CRCHK(dev_alloc_copy(&h->d_slot_role, role.data(), role.size(), h->stream, cfg->device_id));
    }
    std::vector<double> wp, design_rm;
    if (cfg->target_kind == DEMCZ_TARGET_MVNORMAL || cfg->target_kind == DEMCZ_TARGET_ISO_QUAD)
        CRCHK(dev_alloc_copy(&h->d_mu, cfg->mu, (size_t)d, h->stream, cfg->device_id));
    if (cfg->target_kind == DEMCZ_TARGET_MVNORMAL) {
        wp.resize((size_t)d * (d + 1) / 2);
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) wp[(size_t)i * (i + 1) / 2 + j] = cfg->W[i + (size_t)d * j];
        CRCHK(dev_alloc_copy(&h->d_Wp, wp.data(), wp.size(), h->stream, cfg->device_id));
    }
    if (cfg->target_kind == DEMCZ_TARGET_LINREG_SSE) {
        design_rm.resize((size_t)cfg->nobs * d);
        for (int64_t o = 0; o < cfg->nobs; ++o)
            for (int j = 0; j < d; ++j) design_rm[(size_t)o * d + j] = cfg->design[o + cfg->nobs * j];
        CRCHK(dev_alloc_copy(&h->d_design, design_rm.data(), design_rm.size(), h->stream, cfg->device_id));
        CRCHK(dev_alloc_copy(&h->d_y, cfg->yobs, (size_t)cfg->nobs, h->stream, cfg->device_id));
    }
    if (cfg->target_kind == DEMCZ_TARGET_HOST_CALLBACK) {
        CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->dXprop, (size_t)N * d * sizeof(double)));
        CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->dlogu, (size_t)N * sizeof(double)));
    }
    if (cfg->target_kind != DEMCZ_TARGET_HOST_CALLBACK) {
        // waves that run chains in one window launch (every one writes its two counters)
        int64_t waves;
        if (h->lanes == DEMCZ_LAYOUT_SPLIT) {
            // (a two-chain handle's irregular launches run one chain per wave: twice the waves)
            const int64_t wgs = (N + (h->ps_dual ? PS_CHAINS : h->split_per_wg) - 1) / (h->ps_dual ? PS_CHAINS : h->split_per_wg);
            waves = wgs * window_kernel_of(h, LaunchFacts{}).waves;      // (of the launch that is not LIVE: no publisher wave)
        } else if (h->lanes > 1) {
            const int per_wave = 64 / h->lanes;
            const bool lr = h->full_block && cfg->target_kind == DEMCZ_TARGET_LINREG_SSE && d == 10 &&
                            lr16_dynamic_lds<10>(cfg->nobs) <= ML_MAX_DYNAMIC_LDS;      // (uses_lr16: the handle's cfg is not complete yet)
            waves = lr ? ((N + LR16_CHAINS - 1) / LR16_CHAINS) * LR16_WAVES : (N + per_wave - 1) / per_wave;
        } else {
            waves = (N + WINDOW_BS - 1) / WINDOW_BS;
        }
        h->acc_waves = waves;
        h->acc_slots = (int32_t)std::min<int64_t>(4096, std::max<int64_t>(64, (int64_t)(64ll << 20) / (waves * 8)));
        const size_t nb = (size_t)h->acc_slots * (size_t)waves * 2 * sizeof(unsigned int);
        CRCHK(dev_malloc(h->cfg.device_id, (void**)&h->d_acc, nb));
        CRCHK(hipMemsetAsync(h->d_acc, 0, nb, h->stream));
    }
    h->stage_cap = std::max<int64_t>(4096, (int64_t)d * (d + 1) + 64);
    CRCHK(host_malloc((void**)&h->d_stage, (size_t)h->stage_cap * sizeof(double)));
    CRCHK(hipStreamSynchronize(h->stream));   // the host vectors above go out of scope
#undef CRCHK
    *out = h;
    return DEMCZ_OK;
}

// Other replicas publish into this handle's archive from inside their launches: it may only be freed once none of them can
// still be running.  Replica group of this process: every member's streams are drained here and the group is marked dead (its
// other members then only accept demcz_destroy).  Ranks of a communicator: they meet in a reduction behind their launches
// (unless the communicator is dead -- then the archive is NOT freed: a surviving peer's publisher may still be writing it, the
// process is to be restarted anyway), and the IPC mappings of the peers' archives are closed.
static void peer_detach(demcz_handle* h)
{
    if (h->peer_mode == 1 && h->group) {
        PeerGroup* G = h->group;
        if (!G->dead) (void)group_verify(h);          // (what the members have enqueued is completed -- redone if need be -- first)
        for (demcz_handle* m : G->members) {
            if (m->stream) (void)hipStreamSynchronize(m->stream);
            if (m->prod_stream) (void)hipStreamSynchronize(m->prod_stream);
        }
        G->dead = true;
        G->members.erase(std::remove(G->members.begin(), G->members.end(), h), G->members.end());
        for (demcz_handle* m : G->members) { m->n_peers = 0; }
        if (G->members.empty()) delete G;
        h->group = nullptr;
    } else if (h->peer_mode == 3) {
        // (the host has made the ranks meet before this call: demcz_peer_export)
        for (int r = 0; r < DEMCZ_MAX_PEERS; ++r)
            if (h->ipc_mapped[r]) { (void)hipIpcCloseMemHandle(h->ipc_mapped[r]); h->ipc_mapped[r] = nullptr; }
    } else if (h->peer_mode == 2) {
        bool met = false;
        // (every rank destroys its handle at the same point of the program; one that does not -- a handle left to a garbage
        //  collector -- must not hold the others for the full communication deadline: five seconds, then the archive is leaked)
        h->comm_timeout_ms = (h->comm_timeout_ms > 0) ? std::min<int64_t>(h->comm_timeout_ms, 5000) : 5000;
        if (!h->comm_dead && h->comm && h->d_err_all) {
            if (ncclAllReduce(h->d_err_all + 1, h->d_err_all + 1, 1, ncclUint32, ncclMax, h->comm, h->stream) == ncclSuccess)
                met = sync_stream(h, h->stream, "demcz_destroy (peers)") == DEMCZ_OK;
        }
        for (int r = 0; r < DEMCZ_MAX_PEERS; ++r)
            if (h->ipc_mapped[r]) { (void)hipIpcCloseMemHandle(h->ipc_mapped[r]); h->ipc_mapped[r] = nullptr; }
        // ... and once more behind the closing: an exported allocation is only freed when no importer has it mapped any longer
        // (freeing it under a peer's mapping is undefined by the IPC contract, whatever current ROCm makes of it)
        if (met) {
            met = false;
            if (ncclAllReduce(h->d_err_all + 1, h->d_err_all + 1, 1, ncclUint32, ncclMax, h->comm, h->stream) == ncclSuccess)
                met = sync_stream(h, h->stream, "demcz_destroy (peers, mappings closed)") == DEMCZ_OK;
        }
        if (!met && h->archive_fine) h->dZ = nullptr;       // leaked on purpose (see above)
    }
    h->n_peers = 0;
    h->peer_mode = 0;
}

extern "C" int32_t demcz_destroy(demcz_handle* h)
{
    if (!h) return DEMCZ_OK;
    (void)hipSetDevice(h->cfg.device_id);
    // (side streams: a producer kernel for a launch that never came, monitoring checks, a batched exchange.  A sharded handle
    //  waits with its deadline here too -- a peer may have died -- and a dead one has already been given its time to drain)
    // (the copy stream too: a handle destroyed on an error path, or without demcz_get_history_view, may still have D2H copies
    //  of its history in flight into mirrors that are about to go back to the pool)
    for (hipStream_t st : {h->stream, h->prod_stream, h->diag_stream, h->comm_stream, h->hs_stream})
        if (st && !h->comm_dead) (void)sync_stream(h, st, "demcz_destroy");
    peer_detach(h);
    live_release(h);
    free_all(h);
    delete h;
    return DEMCZ_OK;
}

static TargetParams target_params(const demcz_handle* h)
{
    TargetParams tp;
    tp.mu = h->d_mu; tp.Wp = h->d_Wp; tp.c0 = h->cfg.c0;
    tp.design = h->d_design; tp.yobs = h->d_y; tp.nobs = h->cfg.nobs;
    tp.ngrp = h->ngrp; tp.goff = h->d_block_offsets; tp.gstart = h->gstart;
    return tp;
}

static int32_t ensure_scratch(demcz_handle* h, int64_t n)
{
    if (n <= h->scratch_cap) return DEMCZ_OK;
    { int32_t rcq = quiesce_all(h); if (rcq) return rcq; }
    SYNCCHK(h, h->stream);
    if (h->diag_stream) SYNCCHK(h, h->diag_stream);      // a check may still be reading the old buffer
    if (h->prod_stream) SYNCCHK(h, h->prod_stream);      // (the checks of a wave-per-chain handle run there)
    if (h->d_scratch) HIPCHK(h, dev_free(h->cfg.device_id, h->d_scratch));
    h->d_scratch = nullptr; h->scratch_cap = 0;
    HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_scratch, (size_t)n * sizeof(double)));
    h->scratch_cap = n;
    return DEMCZ_OK;
}

static int32_t launch_logp(demcz_handle* h, const double* X, int64_t ldX, int64_t n, double* out)
{
    const TargetParams tp = target_params(h);
    const int bs = 64;
    const dim3 grid((unsigned)((n + bs - 1) / bs));
    switch (h->cfg.target_kind) {
    case DEMCZ_TARGET_MVNORMAL:
        hipLaunchKernelGGL(logp_kernel<TARGET_MVNORMAL>, grid, dim3(bs), 0, h->stream, tp, h->cfg.d, X, ldX, n, out); break;
    case DEMCZ_TARGET_ISO_QUAD:
        hipLaunchKernelGGL(logp_kernel<TARGET_ISO_QUAD>, grid, dim3(bs), 0, h->stream, tp, h->cfg.d, X, ldX, n, out); break;
    case DEMCZ_TARGET_LINREG_SSE:
        hipLaunchKernelGGL(logp_kernel<TARGET_LINREG_SSE>, grid, dim3(bs), 0, h->stream, tp, h->cfg.d, X, ldX, n, out); break;
    case DEMCZ_TARGET_PROGRAM: {
        if (!h->prog_ready) return fail(h, DEMCZ_ERR_STATE, "program target: call demcz_set_program first");
        TargetParams tpv = tp;
        int dv = h->cfg.d;
        void* args[] = {&tpv, &dv, &X, &ldX, &n, &out};
        HIPCHK(h, hipModuleLaunchKernel(h->prog.fn[h->prog_wave ? demcz_prog::WAVE_LOGP : demcz_prog::LANE_LOGP], grid.x, 1, 1, bs, 1, 1, 0, h->stream, args, nullptr));
        break;
    }
    default: return fail(h, DEMCZ_ERR_STATE, "host-callback target: pass logp explicitly");
    }
    HIPCHK(h, hipGetLastError());
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_state(demcz_handle* h, const double* X, const double* logp, const double* Z,
                                   int64_t ldZ, int64_t M0)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (!X || !Z) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_state: X and Z are required");
    if (M0 < 2) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_state: M0 >= 2 needed (two distinct archive rows, demcz.jl:176-179)");
    if (M0 > h->cfg.Mcap || ldZ < M0) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_set_state: M0 exceeds Mcap or ldZ < M0");
    if (!logp && h->cfg.target_kind == DEMCZ_TARGET_HOST_CALLBACK)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_state: host-callback target needs logp");
    if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM && !h->prog_ready)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_state: program target: call demcz_set_program first");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int d = h->cfg.d;
    const int64_t N = h->cfg.N;
    HIPCHK(h, hipMemcpyAsync(h->dX, X, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    {   // parameter-major host matrix -> staging -> row-major archive
        int32_t rcz = ensure_scratch(h, M0 * d);
        if (rcz) return rcz;
        HIPCHK(h, hipMemcpy2DAsync(h->d_scratch, (size_t)M0 * sizeof(double), Z, (size_t)ldZ * sizeof(double),
                                   (size_t)M0 * sizeof(double), (size_t)d, hipMemcpyHostToDevice, h->stream));
        const int64_t tot = M0 * d;
        hipLaunchKernelGGL(append_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ, h->ZS,
                           (int64_t)0, (const double*)h->d_scratch, M0, M0, d);
        HIPCHK(h, hipGetLastError());
        const size_t rest = (size_t)(h->cfg.Mcap - M0) * (size_t)h->ZS;
        if (rest > 0) {
            hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, h->stream,
                               reinterpret_cast<unsigned long long*>(h->dZ + (size_t)M0 * h->ZS), rest, LIVE_SENTINEL);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, hipMemsetAsync(h->d_live_err, 0, 4 * sizeof(unsigned int), h->stream));
    }
    if (logp) {
        HIPCHK(h, hipMemcpyAsync(h->dlp, logp, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        int32_t rc = launch_logp(h, h->dX, N, N, h->dlp);
        if (rc) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->dlp_origin, h->dlp, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    SYNCCHK(h, h->stream);
    h->M = M0;
    h->M_app = M0;
    h->peer_fence = true;
    if (h->no_live && h->rearm_from >= 0) h->rearm_from = 0;      // (a new run numbers its generations from the start again)
    h->live_log.clear();
    h->snap_pending = false;
    h->acc_log.clear();
    { int32_t rcs = rec_scrub(h); if (rcs) return rcs; }
    for (auto& pe : h->pending) if (pe.ev) (void)hipEventDestroy(pe.ev);
    h->pending.clear();
    h->batch_cnt = 0; h->batch_J = -1;
    h->g_done = h->g0;
    h->origin_valid = true;
    h->has_state = true;
    h->proposal_pending = false;
    h->gen_open = false;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_state(demcz_handle* h, double* X, double* logp, double* Z, int64_t ldZ, int64_t* M)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_get_state: no state set");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    {
        int32_t rcv = live_verify(h);
        if (rcv) return rcv;
    }
    const int d = h->cfg.d;
    const int64_t N = h->cfg.N;
    if (X) HIPCHK(h, hipMemcpyAsync(X, h->dX, (size_t)N * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (logp) HIPCHK(h, hipMemcpyAsync(logp, h->dlp, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Z) {
        const int64_t Mall = h->M_app;       // every appended row, visible to proposals yet or not
        if (ldZ < Mall) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_get_state: ldZ < M");
        int32_t rcz = flush_exchanges(h);
        if (rcz) return rcz;
        rcz = ensure_scratch(h, Mall * d);
        if (rcz) return rcz;
        const int64_t tot = Mall * d;
        hipLaunchKernelGGL(export_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->dZ,
                           h->ZS, (int64_t)0, h->d_scratch, Mall, Mall, d);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpy2DAsync(Z, (size_t)ldZ * sizeof(double), h->d_scratch, (size_t)Mall * sizeof(double),
                                   (size_t)Mall * sizeof(double), (size_t)d, hipMemcpyDeviceToHost, h->stream));
    }
    SYNCCHK(h, h->stream);
    if (M) *M = h->M_app;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_archive_pinned(demcz_handle* h, double** Z, int64_t* M)
{
    NOT_DERIVED(h);
    if (!h || !Z || !M) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_get_archive_pinned: no state set");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rc = live_verify(h);
    if (rc) return rc;
    const int d = h->cfg.d;
    const int64_t Mall = h->M_app;
    rc = flush_exchanges(h);
    if (rc) return rc;
    rc = ensure_scratch(h, Mall * d);
    if (rc) return rc;
    double* host = nullptr;
    HIPCHK(h, host_malloc((void**)&host, (size_t)Mall * d * sizeof(double)));
    const int64_t tot = Mall * d;
    hipLaunchKernelGGL(export_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->dZ,
                       h->ZS, (int64_t)0, h->d_scratch, Mall, Mall, d);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host, h->d_scratch, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) {
        (void)host_free(host);
        return fail(h, DEMCZ_ERR_HIP, "demcz_get_archive_pinned: export failed");
    }
    rc = sync_stream(h, h->stream, "demcz_get_archive_pinned");
    if (rc) { (void)host_free(host); return rc; }
    *Z = host;
    *M = Mall;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_history_origin(demcz_handle* h, int64_t g0)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (g0 < 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_history_origin: g0 >= 0");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->live_log.empty()) {          // unverified LIVE launches wrote their history under the old origin
        int32_t rcv = live_verify(h);
        if (rcv) return rcv;
    }
    // slot 0's predecessor is the current log_obj if exactly g0 generations have been run
    h->origin_valid = h->has_state && (h->g_done == g0 || h->g_done == h->g0);
    if (h->has_state)
        HIPCHK(h, hipMemcpyAsync(h->dlp_origin, h->dlp, (size_t)h->cfg.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (h->has_state && h->g_done == h->g0) h->g_done = g0;      // nothing run yet: renumbering only
    h->g0 = g0;
    return DEMCZ_OK;
}

// ---- program targets (demcz_program.hip) ---------------------------------------------------------
namespace {
// Compile `source` into `unit` (or find it in the process-wide cache); needs no device.  What the *_check entry points do, with
// h == nullptr: the message goes where demcz_last_error(NULL) reads it.
int32_t program_compile(demcz_handle* h, int unit, int d, int m, const char* source, const char* options,
                        std::shared_ptr<const demcz_prog::Code>* out = nullptr)
{
    std::shared_ptr<const demcz_prog::Code> code;
    std::string err;
    if (demcz_prog::get_code(d, source, options, unit, code, err, m) != 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, err);
    if (out) *out = code;
    return DEMCZ_OK;
}

// ... and load it on h's device: the module of the unit's kernels (demcz_program.h names them)
int32_t program_load(demcz_handle* h, int unit, int d, int m, const char* source, const char* options, demcz_prog::Module& mod)
{
    std::shared_ptr<const demcz_prog::Code> code;
    if (int32_t rc = program_compile(h, unit, d, m, source, options, &code)) return rc;
    std::string err;
    if (demcz_prog::get_module(code, h->cfg.device_id, mod, err) != 0) return fail(h, DEMCZ_ERR_HIP, err);
    return DEMCZ_OK;
}

// the data of a program: ndata doubles, or none
int32_t data_check(demcz_handle* h, const char* who, const double* data, int64_t ndata)
{
    if (ndata < 0 || (ndata > 0 && !data)) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": need ndata >= 0 and data for ndata > 0");
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_program_check(int32_t d, const char* source, const char* options)
{
    return program_compile(nullptr, demcz_prog::UNIT_ONE_LANE, d, 0, source, options);
}

extern "C" int32_t demcz_program_check_layout(int32_t d, const char* source, const char* options, int32_t lanes_per_chain)
{
    if (lanes_per_chain != 0 && lanes_per_chain != 1 && lanes_per_chain != DEMCZ_LAYOUT_PROGRAM_WAVE)
        return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_program_check_layout: a program target runs one lane per chain: lanes_per_chain must be 0 or 1 "
                                                         "(or DEMCZ_LAYOUT_PROGRAM_WAVE: one wavefront per chain)");
    const int unit = (lanes_per_chain == DEMCZ_LAYOUT_PROGRAM_WAVE) ? demcz_prog::UNIT_WAVE : demcz_prog::UNIT_ONE_LANE;
    return program_compile(nullptr, unit, d, 0, source, options);
}

extern "C" int32_t demcz_set_program(demcz_handle* h, const char* source, const char* options, const double* data, int64_t ndata)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (h->cfg.target_kind != DEMCZ_TARGET_PROGRAM)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_program: the handle was not created with DEMCZ_TARGET_PROGRAM");
    if (h->prog_ready || h->has_state)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_program: a handle takes its program once, before demcz_set_state");
    if (int32_t rc = data_check(h, "demcz_set_program", data, ndata)) return rc;
    // (a handle compiles the unit of ITS layout only: the wave unit is never built for a one-lane handle, nor the reverse)
    demcz_prog::Module mod;
    if (int32_t rc = program_load(h, h->prog_wave ? demcz_prog::UNIT_WAVE : demcz_prog::UNIT_ONE_LANE, h->cfg.d, 0, source, options, mod)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    double* dd = nullptr;
    HIPCHK(h, dev_alloc_copy(&dd, data, (size_t)ndata, h->stream, h->cfg.device_id));
    SYNCCHK(h, h->stream);
    h->d_design = dd;               // (freed with the handle; TargetParams::design / nobs carry it to the kernels)
    h->cfg.nobs = ndata;
    h->prog = mod;
    h->prog_source = source;
    h->prog_options = options ? options : "";
    h->prog_ready = true;
    h->live_wg_cap = -1;            // (wave layout: residency is the program's own kernel's)
    return DEMCZ_OK;
}

// ---- window launch dispatch ------------------------------------------------------------------
// Which kernel a launch runs is decided by window_kernel_of() (below, behind the predicates it is told) and nowhere else.

// Dynamic LDS beyond the default limit is allowed once per (device, kernel): the attribute is per device.
static void allow_dynamic_lds(int device, const WindowKernel& k)
{
    if (!k.big_lds || !k.fn) return;
    static std::mutex mu;
    static std::vector<std::pair<int, const void*>> done;
    const std::pair<int, const void*> key(device, k.fn);
    std::lock_guard<std::mutex> lk(mu);
    if (std::find(done.begin(), done.end(), key) != done.end()) return;
    (void)hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ML_MAX_DYNAMIC_LDS);
    done.push_back(key);
}

// what a crossover launch is told beside WindowParams
static CrossoverParams crossover_params(const demcz_handle* h)
{
    CrossoverParams cp{};
    cp.ncr = h->cr_ncr;
    cp.delta_max = h->cr_delta_max;
    uint32_t sum = 0;
    for (int k = 0; k < CR_MAX_CLASSES; ++k) {
        if (k < h->cr_ncr) sum += (uint32_t)h->cr_weights[k];
        cp.cum[k] = sum;
    }
    cp.counts = h->d_cr_counts;
    return cp;
}

// the one launch of a window kernel: each takes the launch's WindowParams by value
static int32_t launch_kernel(demcz_handle* h, const WindowKernel& k, int64_t blocks, const WindowParams& P)
{
    if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM && !h->prog_ready)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: program target: call demcz_set_program first");
    if (!k.fn && !k.mod) return fail(h, DEMCZ_ERR_STATE, "window launch: target / dimension not built for this handle's layout");
    // (a snooker launch has a second argument; a kernel that takes one never looks at the other)
    SnookerParams sp{h->snooker_lo, h->snooker_hi};
    CrossoverParams cp = crossover_params(h);
    // (an ADAPT crossover launch has a third: where the weights, the spread and the slots of the adaptation are on the device)
    CrossoverAdaptParams ap{};
    if (k.adapt) {
        ap.cum = reinterpret_cast<const uint32_t*>(h->d_cr_adapt + CRA_CUM);
        ap.rsd = reinterpret_cast<const double*>(h->d_cr_adapt + CRA_RSD);
        ap.slots = reinterpret_cast<unsigned long long*>(h->d_cr_adapt + CRA_SLOTS);
        ap.accumulate = h->cr_accumulate_now ? 1 : 0;
    }
    void* args[] = {const_cast<WindowParams*>(&P), k.arm == ARM_CROSSOVER ? (void*)&cp : (void*)&sp, (void*)&ap};
    if (k.mod) {
        HIPCHK(h, hipModuleLaunchKernel(k.mod, (unsigned)blocks, 1, 1, (unsigned)k.threads, 1, 1, (unsigned)k.dyn_lds, h->stream, args, nullptr));
    } else {
        allow_dynamic_lds(h->cfg.device_id, k);
        HIPCHK(h, hipLaunchKernel(k.fn, dim3((unsigned)blocks), dim3((unsigned)k.threads), args, k.dyn_lds, h->stream));
    }
    HIPCHK(h, hipGetLastError());
    if (k.steady) ++h->kernel_counts[0];
    return DEMCZ_OK;
}

// which multi-lane layout is compiled for (target, d, full single block): 0 = none
static int ml_lanes_available(int target_kind, int d, bool full_block, int64_t nobs, int max_blocklen = 0, int nblocks = 1)
{
    if (!full_block) {
        // block updates: every block-step must fit one Philox block per lane: 2 + ceil(b/2) <= L
        if (nblocks > MLB_MAX_BLOCKS) return 0;
        if (target_kind == DEMCZ_TARGET_MVNORMAL) {
            if ((d == 5 || d == 6 || d == 10) && 2 + (max_blocklen + 1) / 2 <= 8) return 8;
            if (d == 20 && 2 + (max_blocklen + 1) / 2 <= 16) return 16;
        }
        return 0;
    }
    if (target_kind == DEMCZ_TARGET_LINREG_SSE && d == 10 &&
        lr16_dynamic_lds<10>(nobs) <= ML_MAX_DYNAMIC_LDS)
        return 16;      // design + y resident in LDS
    // (round 5: any other dimension whose draws fit one Philox block per lane, 2 + ceil(d / 2) <= 16 -- window_kernel_ml with the
    //  sixteen lanes as the spec's sixteen partial sums, the design through L2)
    if (target_kind == DEMCZ_TARGET_LINREG_SSE && d >= 2 && d <= 28) return 16;
    if (target_kind == DEMCZ_TARGET_MVNORMAL) {
        if (d >= 2 && d <= 10) return 8;
        if (d == 20) return 16;
    }
    if (target_kind == DEMCZ_TARGET_ISO_QUAD && d == 10) return 8;
    return 0;
}

// Block updates at d = 20 (C3), split form: sixteen lanes per chain put four chains on a wave and ONE wave on a SIMD at C3's 4096
// chains.  Thirty-two lanes per chain (one parameter a lane, twelve lanes of a chain idle) make it two waves per SIMD that could
// fill each other's LDS waits -- measured (scripts/ab_c3.sh, DEMCZ_MLB_L32=1; bit-exact): 55.2 us per K-window against 45.4:
// the block-step is bound by the instructions it issues, not by their latencies, and the idle lanes' share of them is lost.
// Kept as an experiment switch, off by default.
static bool mlb32_wanted(int64_t)
{
    static const char* env = getenv("DEMCZ_MLB_L32");
    return env && atoi(env) != 0;
}

// split layout (demcz_kernels_pc.h)
static bool pc_available(int target_kind, int d, bool full_block)
{
    if (!full_block) return false;
    // measured per K-window at N=1024 (split vs 8 lanes per chain, fused): d=5 7.0 vs 11.4 us, d=8 7.8 vs 11.6,
    // d=10 11.1 vs 13.5
    if (target_kind == DEMCZ_TARGET_ISO_QUAD) return d == 10;
    // (d = 20: the replicated 210-coefficient whitening does not fit registers -- 63 us per window against
    //  16.7 for the 16-lanes-per-chain kernel, which stays the choice there)
    return target_kind == DEMCZ_TARGET_MVNORMAL && d >= 2 && d <= 10;
}

// the split form of the 16-lane layout (window_kernel_ml<.., REC>): where the replicated consumer does not fit
static bool split_ml_available(int target_kind, int d, bool full_block, int64_t nobs)
{
    if (!full_block) return false;
    if (target_kind == DEMCZ_TARGET_MVNORMAL) return d == 20;
    return target_kind == DEMCZ_TARGET_LINREG_SSE && d == 10 && lr16_dynamic_lds<10>(nobs) <= ML_MAX_DYNAMIC_LDS;
}

// one wave per chain: window_kernel_ps (d <= 5: a pass's draws are one DMA) / window_kernel_pw (C4's d = 20)
// (round 5: every dimension; the isotropic quadratic from d = 6 on -- window_kernel_pw evaluates both targets)
static bool ps_available(int target_kind, int d)
{
    if (target_kind == DEMCZ_TARGET_MVNORMAL) return d >= 2 && d <= PW_D_MAX;
    return target_kind == DEMCZ_TARGET_ISO_QUAD && d >= PW_D_MIN && d <= PW_D_MAX;
}

static int pc_roles(int d) { return ((d == 1) ? 1 : (d + 1) / 2) + 2; }
// doubles of draw record per (generation, chain), and producer lanes per (generation, chain)
static int64_t rec_fields(const demcz_handle* h) { return (h->split_kind == SPLIT_MLB) ? 2 * h->S : (int64_t)h->cfg.d + 2; }
static int64_t rec_roles(const demcz_handle* h) { return (h->split_kind == SPLIT_MLB) ? h->S : pc_roles(h->cfg.d); }

#ifdef DEMCZ_STAMPS
constexpr int64_t DEMCZ_STAMP_WGS = 1 << 16;
#endif

// d = 20, MvNormal, LIVE: candidates and log-densities on the FP64 matrix instruction (demcz_kernels_pw.h, MF).  Built, bit-exact
// (tests/test_gpu_long_oracle.py) -- and measured 4 % SLOWER than the scalar form at C4's shard (6.55-6.60 against 6.2-6.4 us
// per K-window, interleaved runs, profiles/r04i_pw_mfma.txt): 36 matrix instructions at 65 clocks each are the vector rate,
// as DESIGN.md section 9 had costed.  Kept behind DEMCZ_PW_MFMA=1 as the measured experiment; off by default.
static bool pw_matrix_form(const demcz_handle* h)
{
    const char* on = getenv("DEMCZ_PW_MFMA");
    return on && atoi(on) != 0 && h->cfg.d == 20 && h->cfg.target_kind == DEMCZ_TARGET_MVNORMAL;
}

// regular LIVE launches (demcz_kernels_pw.h, REG): K, the distance to the first boundary and the length multiples of five
static bool pw_regular(const WindowParams& P, bool live)
{
    static const bool no_reg = getenv("DEMCZ_NO_PW_REG") != nullptr;
    return live && !no_reg && regular_passes(P.K, P.to_boundary, P.ngen, PS_R);
}

// live: the launch runs through K boundaries whose rows later generations of the SAME launch draw from
static int32_t launch_window_pc(demcz_handle* h, const WindowParams& P, const WindowKernel& k, bool live = false)
{
    const int64_t nbc = (P.N + 63) / 64;
    // 64-lane producer units (the wave-per-chain and replicated consumers' producer, pc_produce, has two lane mappings)
    const bool pc_records = !(h->split_kind == SPLIT_MLB);
    const int64_t units = pc_records ? produce_units(P.N, (int)rec_roles(h), P.rec_fields, P.next_ngen) : nbc * rec_roles(h) * P.next_ngen;
    // producer units per workgroup = waves per workgroup of the instantiation that is launched
    const int upw = k.waves;
    const int64_t blocks = P.consumer_blocks + (units + upw - 1) / upw;
    if (blocks <= 0) return DEMCZ_OK;
    if (h->split_kind == SPLIT_WAVE || h->lr_spec) {
        // consumers whose LIVE launches have the producer half as a kernel of its own beside them: one wave per chain (ps / pw),
        // and the regression target's eight-chains-per-workgroup kernel (its workgroups take a CU's LDS each: producer
        // workgroups of the same grid could only follow them)
        if (h->split_kind == SPLIT_WAVE && P.ZS != ((P.d <= 2) ? 2 : (P.d <= 4) ? 4 : ((P.d + 7) / 8) * 8)) return fail(h, DEMCZ_ERR_STATE, "split layout: archive row stride");
        const int bin = (P.rec_in == h->d_rec[0]) ? 0 : 1, bout = (P.rec_out == h->d_rec[0]) ? 0 : 1;
        const bool one_launch = !live && P.consumer_blocks > 0;     // a short launch: producer workgroups ride in the consumer's grid
        if (units > 0 && one_launch && h->prod_pending[bout]) {
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->prod_done[bout], 0));      // (never two writers of one buffer)
            h->prod_pending[bout] = false;
        }
        if (units > 0 && !one_launch) {
            // the producer half.  Beside a LIVE consumer: on the side stream, behind the consumer that last read
            // the buffer it refills (= everything enqueued on the main stream so far).  Alone (records for THIS window,
            // needed at once): on the main stream.
            hipStream_t ps = h->stream;
            static const bool serial_env = getenv("DEMCZ_PRODUCE_SERIAL") != nullptr;     // diagnosis: producer in front of its consumer's successor, on the main stream
            // (members of a replica group of one process keep to ONE stream each: HIP multiplexes streams over a few hardware
            //  queues, demcz_peer_group has made sure the members' main streams can run at the same time, and a side stream of
            //  one member that shares a hardware queue with another member's main stream was seen to stall the group until the
            //  poll limit -- tests/test_gpu_peer.py after a session that had pooled 30 streams.  Ranks on GPUs of their own
            //  have no such neighbours.)
            if (P.consumer_blocks > 0 && !serial_env && h->peer_mode != 1) {
                if (!h->prod_stream) {
                    HIPCHK(h, stream_acquire(h->cfg.device_id, &h->prod_stream));
                    HIPCHK(h, hipEventCreateWithFlags(&h->prod_gate, hipEventDisableTiming));
                    for (int b = 0; b < 2; ++b) HIPCHK(h, hipEventCreateWithFlags(&h->prod_done[b], hipEventDisableTiming));
                }
                if (h->after_launch_ev) {
                    HIPCHK(h, hipStreamWaitEvent(h->prod_stream, h->after_launch_ev, 0));
                } else {
                    HIPCHK(h, hipEventRecord(h->prod_gate, h->stream));
                    HIPCHK(h, hipStreamWaitEvent(h->prod_stream, h->prod_gate, 0));
                }
                ps = h->prod_stream;
            } else if (h->prod_pending[bout]) {
                HIPCHK(h, hipStreamWaitEvent(h->stream, h->prod_done[bout], 0));      // (never two writers of one buffer)
                h->prod_pending[bout] = false;
            }
            const dim3 pg((unsigned)((units + PRODUCE_WAVES - 1) / PRODUCE_WAVES)), pw(64 * PRODUCE_WAVES);
            // Beside consumers the producers are throttled to PRODUCE_WGS_PER_CU workgroups a CU by an LDS allocation they
            // never touch: more of them only take issue slots from the chain waves (measured); alone they
            // take the whole chip.
            static const size_t throttle_env = getenv("DEMCZ_PRODUCE_LDS") ? (size_t)atol(getenv("DEMCZ_PRODUCE_LDS")) : PRODUCE_THROTTLE_LDS;
            // (regression target: what a consumer workgroup leaves of its CU's LDS holds ONE 8 KB producer workgroup)
            // (two chains to a wave: one 40 KB consumer workgroup per CU at 2048 chains leaves room for three 32 KB producer
            //  workgroups, and the producer has twice the draws to make per launch: 131 against 144 us per launch, profiles/r04j_dual.txt)
            // (wave-per-chain consumers at d > 20 take 70-110 KB of a CU's LDS themselves: the producers' allocation is what is left)
            size_t big_d = throttle_env;
            if (h->split_kind == SPLIT_WAVE && P.d > 20) {
                int plds = 0;       // (program: its own LIVE kernel's static LDS)
                if (h->prog_wave && (!h->prog_ready || hipFuncGetAttribute(&plds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, h->prog.fn[demcz_prog::WAVE_KERNEL + 2 * 1 + 0]) != hipSuccess)) plds = (int)ML_MAX_DYNAMIC_LDS;
                size_t clds = (size_t)plds;
                if (!h->prog_wave) {     // (built-in: the most any of its LIVE forms takes)
                    WindowKernel lk[MAX_LIVE_KERNELS];
                    const int nlk = live_kernels(h, lk);
                    for (int i = 0; i < nlk; ++i) {
                        hipFuncAttributes a{};
                        if (lk[i].fn && hipFuncGetAttributes(&a, lk[i].fn) == hipSuccess) clds = std::max(clds, (size_t)a.sharedSizeBytes);
                    }
                }
                const size_t room = (clds + 4096 < ML_MAX_DYNAMIC_LDS) ? ML_MAX_DYNAMIC_LDS - clds - 4096 : 8192;
                big_d = std::max<size_t>(8192, std::min<size_t>(throttle_env, room));
            }
            const size_t dyn = (ps != h->stream) ? (h->lr_spec ? (size_t)8192 : (h->ps_dual && !getenv("DEMCZ_PRODUCE_LDS")) ? (size_t)32768 : big_d) : 0;
            switch (P.d) {
#define DEMCZ_PRODUCE_CASE(DD) case DD: hipLaunchKernelGGL((produce_kernel<DD>), pg, pw, dyn, ps, P); break;
            DEMCZ_PRODUCE_CASE(2) DEMCZ_PRODUCE_CASE(3) DEMCZ_PRODUCE_CASE(4) DEMCZ_PRODUCE_CASE(5) DEMCZ_PRODUCE_CASE(6) DEMCZ_PRODUCE_CASE(7)
            DEMCZ_PRODUCE_CASE(8) DEMCZ_PRODUCE_CASE(9) DEMCZ_PRODUCE_CASE(10) DEMCZ_PRODUCE_CASE(11) DEMCZ_PRODUCE_CASE(12) DEMCZ_PRODUCE_CASE(13)
            DEMCZ_PRODUCE_CASE(14) DEMCZ_PRODUCE_CASE(15) DEMCZ_PRODUCE_CASE(16) DEMCZ_PRODUCE_CASE(17) DEMCZ_PRODUCE_CASE(18) DEMCZ_PRODUCE_CASE(19)
            DEMCZ_PRODUCE_CASE(20) DEMCZ_PRODUCE_CASE(21) DEMCZ_PRODUCE_CASE(22) DEMCZ_PRODUCE_CASE(23) DEMCZ_PRODUCE_CASE(24) DEMCZ_PRODUCE_CASE(25)
            DEMCZ_PRODUCE_CASE(26) DEMCZ_PRODUCE_CASE(27) DEMCZ_PRODUCE_CASE(28) DEMCZ_PRODUCE_CASE(29) DEMCZ_PRODUCE_CASE(30) DEMCZ_PRODUCE_CASE(31)
            DEMCZ_PRODUCE_CASE(32)
#undef DEMCZ_PRODUCE_CASE
            default: return fail(h, DEMCZ_ERR_STATE, "split layout: dimension not built");
            }
            HIPCHK(h, hipGetLastError());
            if (ps != h->stream) {
                HIPCHK(h, hipEventRecord(h->prod_done[bout], ps));
                h->prod_pending[bout] = true;
            }
        }
        if (P.consumer_blocks > 0) {
            if (h->prod_pending[bin]) {            // this launch's records were made on the side stream
                // A blocking caller (demcz_run_checked) waits for them HERE, on the host: the producer finishes half a launch
                // before the consumer that is running does, so the host is still ahead of the GPU -- and the window launch goes
                // into the queue with nothing in front of it.  A wait enqueued while its event is still pending is a barrier
                // packet between two window kernels (~ 10 us of an idle queue per 1000-generation step, scripts/probes/fixed_cost.py).
                if (h->host_paced) { int32_t rcw = sync_event(h, h->prod_done[bin], "launch_window_pc"); if (rcw) return rcw; }
                else HIPCHK(h, hipStreamWaitEvent(h->stream, h->prod_done[bin], 0));
                h->prod_pending[bin] = false;
            }
            static_assert(PS_CHAINS == LR16_WAVES, "producer units per workgroup of a one-launch grid");
            const int64_t grid = P.consumer_blocks + (one_launch ? (units + PS_CHAINS - 1) / PS_CHAINS : 0);
            return launch_kernel(h, k, grid, P);
        }
        return DEMCZ_OK;
    }
    return launch_kernel(h, k, blocks, P);
}

// Records of the launch (g .. g+ngen-1 against M rows) are in d_rec[rec_cur] when this returns: either
// the previous launch's producer half made them, or a producer-only launch is enqueued now.  Then
// `P` is completed so that this launch's producer half prepares (next_g, next_ngen, next_M).
// Both record buffers hold `gens` generations per (field, chain) afterwards.  demcz_run reserves the most a
// launch of this handle can need before it starts timing or launching (so no allocation, synchronisation or
// memset ever sits between two window launches); pc_prepare only grows them if a caller outruns that.
static int32_t rec_reserve(demcz_handle* h, int64_t gens)
{
    if (gens <= h->rec_cap) return DEMCZ_OK;
    { int32_t rcq = quiesce_all(h); if (rcq) return rcq; }
    SYNCCHK(h, h->stream);
    if (h->prod_stream) SYNCCHK(h, h->prod_stream);
    h->prod_pending[0] = h->prod_pending[1] = false;
    if (h->arena && gens <= h->arena_gens && h->rec_cap == 0) {
        // the arena's buffers (zeroed at create): next to the archive, so that window_kernel_ps2 reaches them by 32-bit offsets
        for (int b = 0; b < 2; ++b) { h->d_rec[b] = h->arena_rec[b]; h->rec_desc[b].valid = false; }
        h->rec_in_arena = true;
        h->rec_cap = h->arena_gens;
        return DEMCZ_OK;
    }
    for (int b = 0; b < 2; ++b) {
        if (h->d_rec[b] && !h->rec_in_arena) HIPCHK(h, dev_free(h->cfg.device_id, h->d_rec[b]));
        h->d_rec[b] = nullptr;
        // (+ REC_PAD doubles: a consumer's last 16-byte chunk fetch may run past its row's last generation)
        const size_t nd = (size_t)gens * (size_t)rec_fields(h) * h->cfg.N + REC_PAD;
        HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_rec[b], nd * sizeof(double)));
        HIPCHK(h, hipMemsetAsync(h->d_rec[b], 0, nd * sizeof(double), h->stream));   // row 0: always a legal index
        h->rec_desc[b].valid = false;
    }
    h->rec_in_arena = false;
    h->rec_cap = gens;
    return DEMCZ_OK;
}

// A launch window_kernel_ps2 can take (demcz_kernels_ps2.h): regular passes, everything reachable by 32-bit offsets.
static bool ps2_applicable(const demcz_handle* h, const WindowParams& P)
{
    static const bool off = getenv("DEMCZ_NO_PS2") != nullptr;
    if (off || h->split_kind != SPLIT_WAVE || h->prog_wave || P.d < 2 || P.d > 5 || !h->arena || !h->rec_in_arena) return false;
    if (P.temperature && (P.temperature < h->arena_temp || P.temperature >= h->arena_temp + h->arena_gens)) return false;
    if (!regular_passes(P.K, P.to_boundary, P.ngen, PS2_R)) return false;
    if (P.chain && (!h->hist_joint || !hist_offsets_32bit(h->cfg.N, h->cfg.d, h->cfg.Gcap))) return false;
    return true;
}

// (lp: the launch's plan, demcz_run_plan.h -- rows join per boundary at the same rate in this launch and in the next)
static int32_t pc_prepare(demcz_handle* h, WindowParams& P, const LaunchPlan& lp)
{
    {
        int32_t rcr = rec_reserve(h, std::max<int64_t>(P.ngen, lp.next_ngen));
        if (rcr) return rcr;
    }
    P.rec_stride = h->rec_cap;
    const int cur = h->rec_cur;
    const int64_t cur_rows = lp.next_rows;
    const int32_t cur_boff = P.K - P.to_boundary;
    auto& dc = h->rec_desc[cur];
    if (!dc.serves(P.g_first, P.ngen, P.M, cur_rows, cur_boff)) {
        WindowParams Q = P;                 // producer-only launch for THIS window
        Q.consumer_blocks = 0;
        Q.rec_out = h->d_rec[cur];
        Q.next_g_first = P.g_first; Q.next_ngen = P.ngen; Q.next_M = P.M; Q.next_rows = cur_rows; Q.next_boff = cur_boff;
        int32_t rc = launch_window_pc(h, Q, window_kernel_of(h, launch_facts(h, &Q, false)));
        if (rc) return rc;
        dc.valid = true; dc.g_first = P.g_first; dc.M = P.M; dc.ngen = P.ngen; dc.rows = cur_rows; dc.boff = cur_boff;
    }
    P.rec_in = h->d_rec[cur];
    const int per_wg = (h->ps_dual && !h->dual_now) ? PS_CHAINS : h->split_per_wg;      // (an irregular launch of a two-chain handle: one chain per wave)
    P.consumer_blocks = (int32_t)((P.N + per_wg - 1) / per_wg);
    P.rec_out = h->d_rec[cur ^ 1];
    P.next_g_first = lp.next_g_first; P.next_ngen = (int32_t)lp.next_ngen; P.next_M = lp.next_M;
    P.next_rows = lp.next_rows; P.next_boff = lp.next_boff;
    auto& dn = h->rec_desc[cur ^ 1];
    dn.valid = lp.next_ngen > 0; dn.g_first = lp.next_g_first; dn.M = lp.next_M; dn.ngen = (int32_t)lp.next_ngen;
    dn.rows = lp.next_rows; dn.boff = lp.next_boff;
    h->rec_cur = cur ^ 1;
    return DEMCZ_OK;
}

// the regression target on the matrix-instruction kernels (demcz_kernels_lr.h): d = 10 with design + y resident in LDS; any other
// regression shape with sixteen lanes per chain runs window_kernel_ml<LINREG_SSE, d, 16>
static bool uses_lr16(const demcz_handle* h)
{
    return h->cfg.target_kind == DEMCZ_TARGET_LINREG_SSE && h->full_block && h->cfg.d == 10 &&
           lr16_dynamic_lds<10>(h->cfg.nobs) <= ML_MAX_DYNAMIC_LDS;
}

// the regression target on sixteen lanes per chain: helper waves share the chain wave's log-density (demcz_kernels_ml.h, COOP) while
// the residuals of a workgroup's four chains fit its LDS
static bool ml_coop(const demcz_handle* h)
{
    static const bool off = getenv("DEMCZ_NO_ML_COOP") != nullptr;
    return ML_LRDPP && !off && h->cfg.target_kind == DEMCZ_TARGET_LINREG_SSE && h->full_block && h->lanes == 16 && !uses_lr16(h) &&
           h->cfg.nobs <= ML_COOP_MAX_OBS;
}

// ---- the kernel of a window launch -----------------------------------------------------------------------------------------------
#define KFN(...) reinterpret_cast<const void*>(&__VA_ARGS__)
// the (LIVE, TEMPER) instantiation of a consumer K<TARGET, D, LIVE, TEMPER>
#define KFN_LT(K, T, D) (f.live ? (f.temper ? KFN(K<T, D, true, true>) : KFN(K<T, D, true, false>)) \
                                : (f.temper ? KFN(K<T, D, false, true>) : KFN(K<T, D, false, false>)))

// window_kernel_mlb<MVNORMAL, D, L, REC, LIVE, QB, GM>; grouped: the sums cut at the block boundaries (full evaluation: the group-start mask)
template <int D, int L, bool REC>
static const void* mlb_fn(bool grouped, bool live)
{
    if constexpr (!REC) {
        return grouped ? KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L, false, false, 0, true>) : KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L>);
    } else {
        if (grouped) return live ? KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L, true, true, 0, true>) : KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L, true, false, 0, true>);
        return live ? KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L, true, true>) : KFN(window_kernel_mlb<TARGET_MVNORMAL, D, L, true, false>);
    }
}

template <bool REC>
static const void* mlb_kernel(const demcz_handle* h, int lanes, bool live)
{
    const bool grouped = h->ngrp > 1;
    switch (h->cfg.d) {
    case 5: return mlb_fn<5, 8, REC>(grouped, live);
    case 6: return mlb_fn<6, 8, REC>(grouped, live);
    case 10: return mlb_fn<10, 8, REC>(grouped, live);
    case 20:
        if constexpr (REC) {
            if (lanes == 32) return mlb_fn<20, 32, true>(grouped, live);
            if (h->mlb_qb == 5)       // four blocks of five: the incremental form
                return live ? KFN(window_kernel_mlb<TARGET_MVNORMAL, 20, 16, true, true, 5>) : KFN(window_kernel_mlb<TARGET_MVNORMAL, 20, 16, true, false, 5>);
        } else {
            if (h->mlb_qb == 5) return KFN(window_kernel_mlb<TARGET_MVNORMAL, 20, 16, false, false, 5>);
        }
        return mlb_fn<20, 16, REC>(grouped, live);
    }
    return nullptr;
}

// The facts of the launch described by P (nullptr: no launch at hand -- untempered, the general forms).  Each predicate is asked
// only for the layout it bears on: some read an environment switch the first time they are called.
static LaunchFacts launch_facts(const demcz_handle* h, const WindowParams* P, bool live)
{
    LaunchFacts f;
    f.live = live;
    f.temper = P && P->temperature != nullptr;
    f.dual = h->dual_now;
    f.snooker = h->snooker_now;
    f.crossover = h->cr_ncr > 0 && !h->snooker_now;
    f.adapt = f.crossover && h->cr_adapt_every > 0;
    if (h->lanes == DEMCZ_LAYOUT_SPLIT) {
        if (h->split_kind == SPLIT_WAVE && !h->prog_wave) {
            f.ps2 = P && ps2_applicable(h, *P);
            f.pw_matrix = h->cfg.d > 5 && pw_matrix_form(h);
            f.pw_reg = P && h->cfg.d > 5 && !f.pw_matrix && pw_regular(*P, live);
        }
    } else if (h->lanes > 1 && h->cfg.target_kind == DEMCZ_TARGET_LINREG_SSE) {
        f.lr16 = uses_lr16(h);
        f.coop = ml_coop(h);
    }
    return f;
}

// THE place that knows which instantiation a handle launches, its workgroup shape and its dynamic LDS.  A pure function of the
// handle's layout and the launch's facts; fn and mod both null: that (layout, target, d) is not built, or the program is not set yet.
static WindowKernel window_kernel_of(const demcz_handle* h, const LaunchFacts& f)
{
    WindowKernel k;
    k.live = f.live;
    k.temper = f.temper;
    const int d = h->cfg.d, tk = h->cfg.target_kind;
    if (f.snooker) {
        // one snooker generation of a one-lane handle (demcz_set_snooker admits no other layout): snooker_kernel<TARGET, D> where
        // the one-lane dispatch specialises the dimension, snooker_kernel_generic<TARGET> otherwise, or the program's own
        k.arm = ARM_SNOOKER;
        k.threads = WINDOW_BS;
        k.waves = 1;
        if (tk == DEMCZ_TARGET_PROGRAM) { if (h->prog_ready) k.mod = h->prog.fn[demcz_prog::LANE_SNOOKER]; }
        else k.fn = snooker_kernel_fn(tk, d, &k.dyn_lds);
        return k;
    }
    if (f.crossover) {
        // crossover generations of a one-lane handle with one block (demcz_set_crossover admits no other): window_kernel_cr<TARGET, D>
        // where the one-lane dispatch specialises the dimension, window_kernel_cr_generic<TARGET> otherwise, or the program's own
        k.arm = ARM_CROSSOVER;
        k.threads = WINDOW_BS;
        k.waves = 1;
        k.adapt = f.adapt;
        if (tk == DEMCZ_TARGET_PROGRAM) { if (h->prog_ready) k.mod = h->prog.fn[f.adapt ? demcz_prog::LANE_CROSSOVER_ADAPT : demcz_prog::LANE_CROSSOVER]; }
        else k.fn = crossover_kernel_fn(tk, d, &k.dyn_lds, f.adapt);
        return k;
    }
    if (h->lanes == DEMCZ_LAYOUT_SPLIT) {
        if (h->lr_spec) {
            k.arm = ARM_LR8S;
            k.threads = 64 * LR16_WAVES;
            k.dyn_lds = lr8s_dynamic_lds<10>(h->cfg.nobs);
            k.big_lds = true;
            k.fn = f.live ? KFN(window_kernel_lr8s<10, true>) : KFN(window_kernel_lr8s<10, false>);
        } else if (h->split_kind == SPLIT_WAVE) {
            k.threads = 64 * (PS_CHAINS + (f.live ? 1 : 0));      // LIVE: chain waves + publisher wave
            if (h->prog_wave) {
                // the program's own wave-per-chain consumer (demcz_program.hip, UNIT_WAVE), with the workgroup shape of the built-in
                // one (its LDS is static)
                k.arm = ARM_PROGRAM_WAVE;
                if (h->prog_ready) k.mod = h->prog.fn[demcz_prog::WAVE_KERNEL + 2 * (f.live ? 1 : 0) + (f.temper ? 1 : 0)];
            } else if (d <= 5) {
                // regular launches: the steady-state kernel -- of a two-chain handle the one with two chains to a wave
                k.arm = (f.dual && f.ps2) ? ARM_PS2D : (!h->ps_dual && f.ps2) ? ARM_PS2 : ARM_PS;
                k.steady = k.arm != ARM_PS;
                switch (d) {
#define DEMCZ_PS_CASE(DD)                                                                                  \
    case DD:                                                                                               \
        k.fn = (k.arm == ARM_PS2D)  ? KFN_LT(window_kernel_ps2d, TARGET_MVNORMAL, DD)                      \
               : (k.arm == ARM_PS2) ? KFN_LT(window_kernel_ps2, TARGET_MVNORMAL, DD)                       \
                                    : KFN_LT(window_kernel_ps, TARGET_MVNORMAL, DD);                       \
        break;
                DEMCZ_PS_CASE(2) DEMCZ_PS_CASE(3) DEMCZ_PS_CASE(4) DEMCZ_PS_CASE(5)
#undef DEMCZ_PS_CASE
                }
            } else {
                // window_kernel_pw (d = 6..32, MvNormal / isotropic quadratic): instantiated in translation units of its own
                k.arm = ARM_PW;
                k.pw_form = (f.live && f.pw_matrix) ? PW_FORM_MATRIX : f.pw_reg ? PW_FORM_REGULAR : PW_FORM_GENERAL;
                k.fn = pw_kernel(tk == DEMCZ_TARGET_ISO_QUAD ? TARGET_ISO_QUAD : TARGET_MVNORMAL, d, f.live, f.temper, k.pw_form);
            }
        } else if (h->split_kind == SPLIT_MLB) {
            k.arm = ARM_MLB_REC;
            k.threads = 64 * h->wpw;
            k.fn = mlb_kernel<true>(h, h->split_lanes, f.live);
        } else if (h->split_kind == SPLIT_ML && tk == DEMCZ_TARGET_LINREG_SSE) {
            k.arm = ARM_LR16_REC;
            k.threads = 64 * LR16_WAVES;
            k.dyn_lds = lr16_dynamic_lds<10>(h->cfg.nobs);
            k.big_lds = true;
            k.fn = f.live ? KFN(window_kernel_lr16<10, true, true>) : KFN(window_kernel_lr16<10, true, false>);
        } else if (h->split_kind == SPLIT_ML) {
            k.arm = ARM_ML_REC;
            k.threads = 64 * h->wpw;
            if (d == 20) k.fn = f.live ? KFN(window_kernel_ml<TARGET_MVNORMAL, 20, 16, true, true>) : KFN(window_kernel_ml<TARGET_MVNORMAL, 20, 16, true, false>);
        } else {
            k.arm = ARM_PC8;
            k.threads = f.live ? 64 * PC8_LIVE_WAVES : 64;        // LIVE: chains wave + publisher wave
            if (tk == DEMCZ_TARGET_ISO_QUAD) {
                if (d == 10) k.fn = KFN_LT(window_kernel_pc8, TARGET_ISO_QUAD, 10);
            } else {
                switch (d) {
#define DEMCZ_PC8_CASE(DD) case DD: k.fn = KFN_LT(window_kernel_pc8, TARGET_MVNORMAL, DD); break;
                DEMCZ_PC8_CASE(2) DEMCZ_PC8_CASE(3) DEMCZ_PC8_CASE(4) DEMCZ_PC8_CASE(5) DEMCZ_PC8_CASE(6) DEMCZ_PC8_CASE(7) DEMCZ_PC8_CASE(8)
                DEMCZ_PC8_CASE(9) DEMCZ_PC8_CASE(10)
#undef DEMCZ_PC8_CASE
                }
            }
        }
        k.waves = k.threads / 64;
    } else if (h->lanes > 1) {
        // fused, 8 / 16 lanes per chain: a workgroup's chain waves hold 64 / lanes chains each
        k.threads = 64;
        k.waves = 1;
        if (!h->full_block) {
            k.arm = ARM_MLB;
            if (tk == DEMCZ_TARGET_MVNORMAL) k.fn = mlb_kernel<false>(h, h->lanes, false);
        } else if (tk == DEMCZ_TARGET_LINREG_SSE && f.lr16) {
            // 16 chains per workgroup of four waves on the 16x16x4 FP64 matrix instruction
            k.arm = ARM_LR16;
            k.threads = 64 * LR16_WAVES;
            k.waves = LR16_WAVES;
            k.dyn_lds = lr16_dynamic_lds<10>(h->cfg.nobs);
            k.big_lds = true;
            if (d == 10) k.fn = KFN(window_kernel_lr16<10, false, false>);
        } else if (tk == DEMCZ_TARGET_LINREG_SSE) {
            // sixteen lanes per chain at any dimension 2..28 (demcz_mlr_dispatch.h); coop: one chain wave + its helper waves
            k.arm = f.coop ? ARM_ML_COOP : ARM_ML;
            k.threads = f.coop ? 64 * ML_COOP_WAVES : 64 * h->wpw;
            k.waves = f.coop ? 1 : h->wpw;
            k.fn = mlr_kernel(d, f.coop);
        } else {
            k.arm = ARM_ML;
            k.threads = 64 * h->wpw;
            k.waves = h->wpw;
            if (tk == DEMCZ_TARGET_ISO_QUAD) {
                if (d == 10) k.fn = KFN(window_kernel_ml<TARGET_ISO_QUAD, 10, 8>);
            } else if (tk == DEMCZ_TARGET_MVNORMAL) {
                switch (d) {
#define DEMCZ_ML8_CASE(DD) case DD: k.fn = KFN(window_kernel_ml<TARGET_MVNORMAL, DD, 8>); break;
                DEMCZ_ML8_CASE(2) DEMCZ_ML8_CASE(3) DEMCZ_ML8_CASE(4) DEMCZ_ML8_CASE(5) DEMCZ_ML8_CASE(6) DEMCZ_ML8_CASE(7) DEMCZ_ML8_CASE(8)
                DEMCZ_ML8_CASE(9) DEMCZ_ML8_CASE(10)
#undef DEMCZ_ML8_CASE
                case 20: k.fn = KFN(window_kernel_ml<TARGET_MVNORMAL, 20, 16>); break;
                }
            }
        }
    } else {
        // one lane per chain: window_kernel<TARGET, D, FULL> where the dimension is specialised, window_kernel_generic<TARGET> otherwise
        k.arm = ARM_ONE_LANE;
        k.threads = WINDOW_BS;
        k.waves = 1;
#define DEMCZ_ONE_LANE_CASE(T, DD) case DD: k.fn = h->full_block ? KFN(window_kernel<T, DD, true>) : KFN(window_kernel<T, DD, false>); break;
#define DEMCZ_GENERIC_CASE(T) default: k.fn = KFN(window_kernel_generic<T>); k.dyn_lds = (size_t)(3 * d + 1) * WINDOW_BS * sizeof(double); break;
        switch (tk) {
        case DEMCZ_TARGET_MVNORMAL:
            switch (d) {
            DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 2) DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 3) DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 4)
            DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 5) DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 8) DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 10)
            DEMCZ_ONE_LANE_CASE(TARGET_MVNORMAL, 20) DEMCZ_GENERIC_CASE(TARGET_MVNORMAL)
            }
            break;
        case DEMCZ_TARGET_ISO_QUAD:
            switch (d) { DEMCZ_ONE_LANE_CASE(TARGET_ISO_QUAD, 10) DEMCZ_GENERIC_CASE(TARGET_ISO_QUAD) }
            break;
        case DEMCZ_TARGET_LINREG_SSE:
            switch (d) { DEMCZ_ONE_LANE_CASE(TARGET_LINREG_SSE, 10) DEMCZ_ONE_LANE_CASE(TARGET_LINREG_SSE, 26) DEMCZ_GENERIC_CASE(TARGET_LINREG_SSE) }
            break;
        case DEMCZ_TARGET_PROGRAM:
            // the program's own window_kernel<TARGET_PROGRAM, d, FULL> (demcz_program.hip), from its module
            if (h->prog_ready) k.mod = h->prog.fn[h->full_block ? demcz_prog::LANE_FULL : demcz_prog::LANE_BLOCKS];
            break;
        default: break;       // (host-callback target: demcz_propose / demcz_accept_commit, no window kernel)
        }
#undef DEMCZ_ONE_LANE_CASE
#undef DEMCZ_GENERIC_CASE
    }
    return k;
}
#undef KFN_LT
#undef KFN

// The LIVE kernels a handle of the split layout may launch: every tempered / untempered form its consumer has.  (Wave-per-chain,
// d >= 6: the matrix form too where it is built, whether or not DEMCZ_PW_MFMA asks for it.)  A form that should exist and is not
// built comes back with fn == nullptr.
static int live_kernels(const demcz_handle* h, WindowKernel out[MAX_LIVE_KERNELS])
{
    LaunchFacts forms[3];
    int nf = 1;
    forms[0].live = true;
    if (h->split_kind == SPLIT_WAVE && !h->prog_wave && !h->lr_spec) {
        if (h->cfg.d > 5) {
            forms[1] = forms[2] = forms[0];
            forms[1].pw_reg = true;
            forms[2].pw_matrix = true;
            nf = 3;
        } else if (h->ps_dual) {      // (its LIVE launches are all of the two-chain kernel)
            forms[0].ps2 = forms[0].dual = true;
        } else {
            forms[1] = forms[0];
            forms[1].ps2 = true;
            nf = 2;
        }
    }
    int n = 0;
    for (int i = 0; i < nf; ++i)
        for (int t = 0; t < 2; ++t) {
            forms[i].temper = t != 0;
            const WindowKernel k = window_kernel_of(h, forms[i]);
            if (forms[i].pw_matrix && !k.fn) continue;                                  // (built at one target and dimension only)
            if (n > 0 && out[n - 1].fn == k.fn && out[n - 1].mod == k.mod) continue;    // (a kernel with no tempered form of its own)
            out[n++] = k;
        }
    return n;
}

static int32_t launch_window(demcz_handle* h, const WindowParams& P, bool live = false)
{
    const WindowKernel k = window_kernel_of(h, launch_facts(h, &P, live));
    if (P.consumer_blocks > 0 || h->lanes != DEMCZ_LAYOUT_SPLIT) h->last_kernel = k;      // (not the producer-only launches)
    if (h->snap_pending) {
        // the redo snapshot of the state (demcz_run): window_kernel_ps2 writes it as it loads the state -- two 5 us copy launches
        // less in front of every autostop slab -- any other kernel gets the copies
        h->snap_pending = false;
        if (k.steady) {
            WindowParams Q = P;
            Q.safe_X = h->d_safe_X;
            Q.safe_lp = h->d_safe_lp;
            return launch_window(h, Q, live);
        }
        HIPCHK(h, hipMemcpyAsync(h->d_safe_X, h->dX, (size_t)h->cfg.N * h->cfg.d * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_safe_lp, h->dlp, (size_t)h->cfg.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    int32_t rc;
    if (h->lanes == DEMCZ_LAYOUT_SPLIT) {
        rc = launch_window_pc(h, P, k, live);
    } else {
        const int per_wg = k.waves * (64 / h->lanes);      // chains per workgroup
        rc = launch_kernel(h, k, (P.N + per_wg - 1) / per_wg, P);
    }
    if (rc) return rc;
    ++h->launches;
    return DEMCZ_OK;
}

// Synchronous exchange (lag == 0) of a sharded run: all-gather the end-of-window states and
// scatter them into every replica of the archive; the next window sees them.
static int32_t append_after_window(demcz_handle* h)
{
    const int d = h->cfg.d;
    const int64_t N = h->cfg.N;
    if (h->comm) {   // also at nranks == 1, so the collective path is exercised on a one-GPU box
        const int64_t total = N * h->nranks;
        if (h->M_app + total > h->cfg.Mcap) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_run: Z capacity exceeded");
        { int32_t rcs = maybe_stall(h, h->stream); if (rcs) return rcs; }
        NCCLCHK(h, ncclAllGather(h->dX, h->d_gather, (size_t)N * d, ncclDouble, h->comm, h->stream));
        const int64_t tot = total * d;
        hipLaunchKernelGGL(append_gathered_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ,
                           h->ZS, h->M_app, h->d_gather, N, h->nranks, d);
        HIPCHK(h, hipGetLastError());
        h->M_app += total;
        h->M = h->M_app;
    }
    return DEMCZ_OK;
}

// Deferred exchange (lag E >= 1) of a sharded run: the snapshots of up to E boundaries travel in one
// all-gather on a side stream while the next windows compute; the rows become visible E windows after
// the batch closes (see demcz_set_append_lag), by which time the compute stream waits on the event.
static int32_t exchange_batch(demcz_handle* h)
{
    if (h->batch_cnt == 0) return DEMCZ_OK;
    const int d = h->cfg.d, cnt = h->batch_cnt, buf = h->batch_buf;
    const int64_t N = h->cfg.N;
    hipEvent_t ready;
    HIPCHK(h, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(ready, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm_stream, ready, 0));
    HIPCHK(h, hipEventDestroy(ready));
    { int32_t rcs = maybe_stall(h, h->comm_stream); if (rcs) return rcs; }
    NCCLCHK(h, ncclAllGather(h->d_send[buf], h->d_recv[buf], (size_t)N * d * cnt, ncclDouble, h->comm_side, h->comm_stream));
    const int64_t tot = N * d * cnt * h->nranks;
    hipLaunchKernelGGL(append_batch_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->comm_stream, h->dZ, h->ZS,
                       h->batch_base, (const double*)h->d_recv[buf], N, h->nranks, cnt, d);
    HIPCHK(h, hipGetLastError());
    hipEvent_t done;
    HIPCHK(h, hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(done, h->comm_stream));
    h->pending.back().ev = done;                       // the entry that covers this batch
    h->pending.back().xseq = ++h->xseq;
    if (!h->xdone) {
        HIPCHK(h, host_malloc((void**)&h->xdone, sizeof(long long)));
        *h->xdone = 0;
    }
    hipLaunchKernelGGL(mark_kernel, dim3(1), dim3(1), 0, h->comm_stream, h->xdone, (long long)h->xseq);
    HIPCHK(h, hipGetLastError());
    h->buf_xseq[buf] = h->xseq;
    HIPCHK(h, hipEventRecord(h->buf_done[buf], h->comm_stream));
    h->batch_cnt = 0;
    h->batch_buf ^= 1;
    h->batch_J = -1;                                   // later boundaries of the same batch open a new entry
    return DEMCZ_OK;
}

// Rows whose visibility generation has been reached join the part of the archive proposals draw from.
static int32_t admit_pending(demcz_handle* h, int64_t g)
{
    while (!h->pending.empty() && h->pending.front().visible_from <= g) {
        auto pe = h->pending.front();
        if (pe.ev) {
            // (a blocking caller waits on the host: see launch_window_pc -- the exchange of a batch has the whole next batch to
            //  finish, and the batch after that is only enqueued now)
            if (h->host_paced && h->xdone) {
                volatile long long* xd = h->xdone;
                const long long need = (long long)pe.xseq;
                int32_t rcw = wait_deadline(h, [xd, need]() { return (*xd >= need) ? hipSuccess : hipErrorNotReady; }, "admit_pending (exchange of a batch)");
                if (rcw) return rcw;
            }
            else HIPCHK(h, hipStreamWaitEvent(h->stream, pe.ev, 0));
            HIPCHK(h, hipEventDestroy(pe.ev));
            h->xseq_waited = std::max(h->xseq_waited, pe.xseq);      // (the side stream runs its exchanges in order)
        }
        h->M = pe.M_after;
        h->pending.pop_front();
    }
    return DEMCZ_OK;
}

// Everything appended so far is in the archive when this returns (used before reading Z back).
static int32_t flush_exchanges(demcz_handle* h)
{
    if (h->comm && h->lag > 0) {
        int32_t rc = exchange_batch(h);
        if (rc) return rc;
        for (auto& pe : h->pending)
            if (pe.ev) HIPCHK(h, hipStreamWaitEvent(h->stream, pe.ev, 0));
    }
    return DEMCZ_OK;
}

// A LIVE launch that gave up waiting for a row leaves a word behind; results after it are void.
static int32_t check_live_err(demcz_handle* h)
{
    unsigned int e[4] = {0, 0, 0, 0};
    if (!h->d_live_err) return DEMCZ_OK;         // (the scratch handles of the *_array diagnostics run no chains)
    if (h->err_clean) return DEMCZ_OK;           // (read as zero since the last LIVE launch: a blocking 16-byte copy less per call)
    HIPCHK(h, hipMemcpy(e, h->d_live_err, sizeof(e), hipMemcpyDeviceToHost));
    if (!e[0]) h->err_clean = true;
    if (e[0])
        return fail(h, DEMCZ_ERR_HIP, "demcz_run: an archive row appended inside the launch never became visible (LIVE hand-off): "
                                      "generation " + std::to_string(e[1]) + " of the launch, row " + std::to_string(e[2]) +
                                      ", workgroup " + std::to_string(e[3]) + ", rows appended " + std::to_string(h->M_app));
    return DEMCZ_OK;
}

// What a failed hand-off leaves behind is undone: X, log_obj, M go back to the state before the first unverified
// demcz_run call, the rows written since read as unwritten again, the error word is cleared, and the handle stops
// using LIVE launches.  Returns the calls made since (for live_verify to redo).
static int32_t live_rollback(demcz_handle* h, std::vector<demcz_handle::RunCall>& calls)
{
    calls.swap(h->live_log);
    h->live_log.clear();
    const int64_t N = h->cfg.N;
    const int d = h->cfg.d;
    SYNCCHK(h, h->stream);
    if (h->diag_stream) SYNCCHK(h, h->diag_stream);
    if (h->prod_stream) SYNCCHK(h, h->prod_stream);
    if (!h->snap_pending) {              // (still pending: nothing was launched since, the state is the snapshot)
        HIPCHK(h, hipMemcpyAsync(h->dX, h->d_safe_X, (size_t)N * d * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->dlp, h->d_safe_lp, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    h->snap_pending = false;
    if (h->M_app > h->safe_M_app) {
        const size_t rest = (size_t)(h->M_app - h->safe_M_app) * (size_t)h->ZS;
        hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, h->stream,
                           reinterpret_cast<unsigned long long*>(h->dZ + (size_t)h->safe_M_app * h->ZS), rest, LIVE_SENTINEL);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemsetAsync(h->d_live_err, 0, 4 * sizeof(unsigned int), h->stream));
    SYNCCHK(h, h->stream);
    h->peer_fence = true;
    // Where the redo may go LIVE again: behind the demcz_run call that holds the generation whose row never arrived.  The row
    // says which boundary it belongs to -- rows [safe_M_app + j * rows, + rows) are boundary j since the verified point, appended
    // after generation (safe_g_done / K + 1 + j) * K -- and the wave that gave up was working on a generation behind it.  No row
    // on record (the launch found the word already set; a kernel that does not note it): behind everything enqueued so far.
    int64_t from = h->g_done;
    if (h->fail_row_hint != 0xffffffffu && (int64_t)h->fail_row_hint >= h->safe_M_app && (int64_t)h->fail_row_hint < h->M_app) {
        const int64_t rows = h->cfg.N * ((h->comm || h->peer_mode != 0) ? h->nranks : 1);
        const int64_t j = ((int64_t)h->fail_row_hint - h->safe_M_app) / rows;
        from = std::min<int64_t>(from, (h->safe_g_done / h->cfg.K + 1 + j) * (int64_t)h->cfg.K + 1);
    }
    h->fail_row_hint = 0xffffffffu;
    h->M = h->safe_M;
    h->M_app = h->safe_M_app;
    h->g_done = h->safe_g_done;
    while (!h->acc_log.empty() && h->acc_log.back().g_last > h->safe_g_done) h->acc_log.pop_back();
    { int32_t rcs = rec_scrub(h); if (rcs) return rcs; }
    h->no_live = true;
    h->rearm_from = -1;
    if (h->peer_mode != 1 && h->peer_mode != 3 && h->live_rearms_left > 0) {      // (a replica group re-arms as a whole: group_verify)
        --h->live_rearms_left;
        h->rearm_from = from;
    }
    // (a fault a test injected has fired: the redo's LIVE launches run with the handle's own poll limit)
    h->live_fault_polls = 0;
    live_release(h);
    ++h->live_redos;
    return DEMCZ_OK;
}

// The handle tries LIVE launches again (see demcz_handle::live_rearms_left).  Called at a point where everything enqueued so far
// ran one launch per K-window -- nothing of it can have failed -- and every rank of a sharded run is at the same call with the
// same decision to try (it follows from the max-reduced error word and the min-reduced row of live_failed).  Whether a rank CAN
// -- its share of the device's LIVE budget may have gone to another handle of its process meanwhile -- is agreed by a
// min-reduction: either all ranks hand rows over inside their launches again or none does (a rank exchanging through
// ncclAllGather while its peers publish and poll would stall all of them until the communicator's deadline).  The ranks meet
// once more, stream-ordered, before the first launch that publishes (peer_fence, set by the rollback).
static int32_t live_try_rearm(demcz_handle* h)
{
    h->rearm_from = -1;
    h->no_live = false;
    unsigned int ok = live_span(h) > 0 ? 1u : 0u;
    if (h->peer_mode == 2 && h->comm && h->d_err_all) {
        HIPCHK(h, hipMemcpyAsync(h->d_err_all + 2, &ok, sizeof(ok), hipMemcpyHostToDevice, h->stream));
        NCCLCHK(h, ncclAllReduce(h->d_err_all + 2, h->d_err_all + 2, 1, ncclUint32, ncclMin, h->comm, h->stream));
        SYNCCHK(h, h->stream);
        HIPCHK(h, hipMemcpy(&ok, h->d_err_all + 2, sizeof(ok), hipMemcpyDeviceToHost));
    }
    if (!ok) {
        h->no_live = true;
        live_release(h);
        return DEMCZ_OK;
    }
    ++h->live_rearms;
    if (getenv("DEMCZ_DEBUG_LIVE")) fprintf(stderr, "[demcz] rank %d: LIVE launches re-armed (%d re-arms left)\n", h->rank, (int)h->live_rearms_left);
    return DEMCZ_OK;
}

// Did a LIVE launch since the last verified point give up waiting for a row?  The stream is drained first.  With the ranks of a
// communicator publishing into each other's replicas (peer_mode 2) the answer must be the SAME on every rank -- a rank whose own
// waits all succeeded still has to join the others' redo, which exchanges rows through RCCL -- so the error words are
// max-reduced over the communicator (every rank makes the same calls in the same order, so every rank is here together).
static int32_t live_failed(demcz_handle* h, bool& failed)
{
    failed = false;
    SYNCCHK(h, h->stream);
    unsigned int e[4] = {0, 0, 0, 0};
    if (h->peer_mode == 2 && !h->no_live && h->comm) {
        NCCLCHK(h, ncclAllReduce(h->d_live_err, h->d_err_all, 1, ncclUint32, ncclMax, h->comm, h->stream));
        SYNCCHK(h, h->stream);
        HIPCHK(h, hipMemcpy(e, h->d_err_all, sizeof(unsigned int), hipMemcpyDeviceToHost));
    } else if (h->pinned_err && h->pinned_err_launches == h->launches) {
        // (copied behind the last window launch, and the stream has been drained since: demcz_run_checked)
        std::memcpy(e, h->pinned_err, sizeof(e));
    } else {
        HIPCHK(h, hipMemcpy(e, h->d_live_err, sizeof(e), hipMemcpyDeviceToHost));
    }
    h->pinned_err_launches = -1;
    failed = e[0] != 0u;
    if (!failed && h->peer_mode != 2) h->err_clean = true;
    if (failed) {
        // which row: what live_rollback places the re-arming point by.  Ranks of a communicator need the SAME point: the smallest
        // row any of them has on record (0xffffffff: none on this rank -- its own waits all succeeded, or the wave that gave up
        // could not say).  Every rank knows `failed` from the reduction above, so every rank is in this one too.
        unsigned int row = 0xffffffffu;
        if (h->peer_mode == 2 && !h->no_live && h->comm) {
            unsigned int le[4] = {0, 0, 0, 0};
            HIPCHK(h, hipMemcpy(le, h->d_live_err, sizeof(le), hipMemcpyDeviceToHost));
            if (le[0] && le[0] == 1u) row = le[2];
            HIPCHK(h, hipMemcpyAsync(h->d_err_all + 2, &row, sizeof(row), hipMemcpyHostToDevice, h->stream));
            NCCLCHK(h, ncclAllReduce(h->d_err_all + 2, h->d_err_all + 2, 1, ncclUint32, ncclMin, h->comm, h->stream));
            SYNCCHK(h, h->stream);
            HIPCHK(h, hipMemcpy(&row, h->d_err_all + 2, sizeof(row), hipMemcpyDeviceToHost));
        } else if (e[0] == 1u) {           // (the word a wave's compare-and-swap wrote; a test's pre-set word has no row behind it)
            row = e[2];
        }
        h->fail_row_hint = row;
        if (getenv("DEMCZ_DEBUG_LIVE")) {
            unsigned int le[4] = {0, 0, 0, 0};
            (void)hipMemcpy(le, h->d_live_err, sizeof(le), hipMemcpyDeviceToHost);
            fprintf(stderr, "[demcz] rank %d: hand-off failed: word %#x, generation %u of its launch, row %u, workgroup %u; verified point: g %lld, M %lld; enqueued: g %lld, M %lld; launches %lld\n",
                    h->rank, le[0], le[1], le[2], le[3], (long long)h->safe_g_done, (long long)h->safe_M_app, (long long)h->g_done, (long long)h->M_app, (long long)h->launches);
        }
    }
    return DEMCZ_OK;
}

// Every entry point that hands results to the caller goes through here: the stream is drained, and if a LIVE
// launch since the last verification gave up waiting for a row, everything since then is redone with one launch
// per K-window (bit-identical results; the handle stays in that mode).  DEMCZ_OK afterwards means the results are valid.
static int32_t live_verify(demcz_handle* h)
{
    DEADCHK(h);
    if (h->peer_mode == 1) return group_verify(h);
    if (h->live_log.empty() || h->replaying) return check_live_err(h);
    bool failed = false;
    int32_t rc = live_failed(h, failed);
    if (rc) return rc;
    if (!failed) { h->live_log.clear(); return DEMCZ_OK; }
    if (h->peer_mode == 3) {
        h->no_live = true;
        return fail(h, DEMCZ_ERR_STATE, "a row another rank should have published never became visible (in-launch hand-off, host-mediated IPC peers): "
                                        "results since the last verified point are void on every rank");
    }
    // The redo: back to the verified point, the logged calls again.  They run one launch per K-window up to the call that holds
    // the generation whose row never came; a call that starts behind it may go LIVE again (live_try_rearm, in demcz_run) -- its
    // launches are logged like any others, against the SAME verified point (`replaying`: no new snapshot), and should one of them
    // fail too the whole list is redone once more.  Bounded: every failure takes one of the handle's re-arms, and without one
    // left the redo cannot fail.
    std::vector<demcz_handle::RunCall> calls, dropped;
    rc = live_rollback(h, calls);
    if (rc) return rc;
    for (;;) {
        h->replaying = true;
        for (const auto& c : calls) {
            rc = demcz_run(h, c.g_from, c.g_to, c.gamma, c.tempered ? c.temperature.data() : nullptr);
            if (rc) break;
        }
        h->replaying = false;
        if (rc) return rc;
        if (h->live_log.empty()) break;
        rc = live_failed(h, failed);
        if (rc) return rc;
        if (!failed) { h->live_log.clear(); return DEMCZ_OK; }
        rc = live_rollback(h, dropped);
        if (rc) return rc;
    }
    SYNCCHK(h, h->stream);
    return check_live_err(h);
}

// ---- replica groups of one process (demcz_peer_group) --------------------------------------------------------------------------
// The calls of `calls[m]` (the same list for every member) executed for all members in lockstep, one launch per K-window, the
// boundary rows of all members appended to every replica in rank order from the members' own state buffers: what the
// in-launch hand-off does, without it.  The host waits for every phase -- this is the fall-back, not the product path.
static int32_t group_execute(PeerGroup* G, const std::vector<std::vector<demcz_handle::RunCall>>& calls)
{
    const size_t ncall = calls.empty() ? 0 : calls[0].size();
    for (const auto& cm : calls)
        if (cm.size() != ncall) return DEMCZ_ERR_STATE;
    auto sync_all = [&]() -> int32_t {
        for (demcz_handle* m : G->members) {
            if (hipStreamSynchronize(m->stream) != hipSuccess) return fail(m, DEMCZ_ERR_HIP, "replica group: stream synchronisation failed");
            if (m->prod_stream && hipStreamSynchronize(m->prod_stream) != hipSuccess) return fail(m, DEMCZ_ERR_HIP, "replica group: stream synchronisation failed");
        }
        return DEMCZ_OK;
    };
    int32_t rc = DEMCZ_OK;
    for (demcz_handle* m : G->members) { m->replaying = true; m->external_append = true; }
    for (size_t ic = 0; ic < ncall && rc == DEMCZ_OK; ++ic) {
        const auto& c0 = calls[0][ic];
        for (size_t mi = 0; mi < G->members.size(); ++mi)
            if (calls[mi][ic].g_from != c0.g_from || calls[mi][ic].g_to != c0.g_to) rc = DEMCZ_ERR_STATE;
        if (rc) break;
        const int K = G->members[0]->cfg.K;
        for (int64_t g = c0.g_from; g <= c0.g_to && rc == DEMCZ_OK;) {
            const int64_t w_end = std::min<int64_t>(boundary_at_or_after(g, K), c0.g_to);       // (plan_launch's schedule with span 0)
            for (size_t mi = 0; mi < G->members.size() && rc == DEMCZ_OK; ++mi) {
                const auto& c = calls[mi][ic];
                rc = demcz_run(G->members[mi], g, w_end, c.gamma, c.tempered ? c.temperature.data() + (g - c.g_from) : nullptr);
            }
            if (rc == DEMCZ_OK) rc = sync_all();
            if (rc == DEMCZ_OK && w_end % K == 0) {
                for (demcz_handle* m : G->members)
                    for (demcz_handle* src : G->members) {
                        if (rc == DEMCZ_OK) rc = demcz_append_rows_device(m, src->dX, src->cfg.N, src->cfg.N);
                        if (rc != DEMCZ_OK && m != src && m->err.empty()) m->err = src->err;
                    }
                if (rc == DEMCZ_OK) rc = sync_all();
            }
            g = w_end + 1;
        }
    }
    for (demcz_handle* m : G->members) { m->replaying = false; m->external_append = false; m->rec_desc[0].valid = m->rec_desc[1].valid = false; }
    return rc;
}

// Verification for a member of a replica group = for the whole group (one host thread drives all members, and a member's
// results depend on every other member's launches having run): all streams are drained, all error words looked at.
static int32_t group_verify(demcz_handle* h)
{
    PeerGroup* G = h->group;
    if (!G || G->busy || h->replaying) return check_live_err(h);
    if (G->dead) {      // (a member is gone; it verified the whole group on its way out, so what is there is valid)
        if (h->live_log.empty()) return check_live_err(h);
        return fail(h, DEMCZ_ERR_STATE, "a member of this handle's replica group has been destroyed");
    }
    bool any_log = false;
    for (demcz_handle* m : G->members) any_log = any_log || !m->live_log.empty();
    if (!any_log) return check_live_err(h);
    for (demcz_handle* m : G->members)
        if (m->live_log.size() != h->live_log.size())
            return fail(h, DEMCZ_ERR_STATE, "replica group: every member must be given the same demcz_run calls before any member's results are asked for");
    G->busy = true;
    struct Unbusy { PeerGroup* g; ~Unbusy() { g->busy = false; } } unbusy{G};
    bool failed = false;
    for (demcz_handle* m : G->members) {
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (m->prod_stream) HIPCHK(m, hipStreamSynchronize(m->prod_stream));
    }
    for (demcz_handle* m : G->members) {
        unsigned int e[4] = {0, 0, 0, 0};
        HIPCHK(m, hipMemcpy(e, m->d_live_err, sizeof(e), hipMemcpyDeviceToHost));
        failed = failed || e[0] != 0u;
        if (e[0] && getenv("DEMCZ_DEBUG_LIVE"))
            fprintf(stderr, "[demcz] replica %d of %d: hand-off timed out at generation %u of its launch, row %u, workgroup %u (M_app %lld, M %lld, launches %lld, live_claimed %d)\n",
                    m->rank, m->nranks, e[1], e[2], e[3], (long long)m->M_app, (long long)m->M, (long long)m->launches, (int)m->live_claimed);
    }
    if (!G->failed && !failed) {
        for (demcz_handle* m : G->members) m->live_log.clear();
        return DEMCZ_OK;
    }
    std::vector<std::vector<demcz_handle::RunCall>> calls(G->members.size());
    if (!G->failed) {
        // first failure: every member goes back to the state before its first unverified call
        for (size_t mi = 0; mi < G->members.size(); ++mi) {
            int32_t rc = live_rollback(G->members[mi], calls[mi]);
            if (rc) { if (G->members[mi] != h) h->err = G->members[mi]->err; return rc; }
        }
        G->failed = true;
    } else {
        // the group already runs deferred: the logged calls have not been executed at all
        for (size_t mi = 0; mi < G->members.size(); ++mi) { calls[mi].swap(G->members[mi]->live_log); G->members[mi]->live_log.clear(); }
    }
    int32_t rc = group_execute(G, calls);
    if (rc) {
        if (h->err.empty()) for (demcz_handle* m : G->members) if (!m->err.empty()) { h->err = m->err; break; }
        if (rc == DEMCZ_ERR_STATE && h->err.empty()) h->err = "replica group: the members were not given the same calls";
        return rc;
    }
    for (demcz_handle* m : G->members) m->g_done = calls[0].empty() ? m->g_done : calls[0].back().g_to;
    if (G->failed && !G->lockstep_only && G->rearms_left > 0) {
        // everything logged has been executed in lockstep, every member is at the same verified point: the group hands its rows
        // over inside the launches again from the next call on (bounded: see demcz_handle::live_rearms_left)
        --G->rearms_left;
        G->failed = false;
        for (demcz_handle* m : G->members) { m->no_live = false; m->rearm_from = -1; m->live_rearms_left = G->rearms_left; ++m->live_rearms; }
    }
    return check_live_err(h);
}

// The consumer workgroups of a LIVE launch wait for each other's rows, so all of them must be resident at
// once.  Capacity = what the occupancy query gives for the LIVE instantiation of this handle's kernel
// (both accept variants) x CUs; half of it is used, which leaves room for the producer half, for other
// streams' kernels and for the query being one block per CU optimistic (MI355X_MICROARCH.md, residency).
// Beyond that the split layout falls back to one launch per K-window.
static int blocks_per_cu(int device, const WindowKernel& k)
{
    int n = 0;
    if (k.mod) return hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.mod, k.threads, k.dyn_lds) == hipSuccess ? n : 0;
    if (!k.fn) return 0;
    allow_dynamic_lds(device, k);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, k.threads, k.dyn_lds) == hipSuccess ? n : 0;
}

static int64_t live_wg_capacity(demcz_handle* h)
{
    if (h->live_wg_cap >= 0) return h->live_wg_cap;
    // the program's own LIVE kernels: a register-hungry user function lowers what fits a CU (nothing is known, and nothing
    // is remembered, before demcz_set_program)
    if (h->prog_wave && !h->prog_ready) return 0;
    WindowKernel lk[MAX_LIVE_KERNELS];
    const int nlk = live_kernels(h, lk);
    int per_cu = blocks_per_cu(h->cfg.device_id, lk[0]);
    for (int i = 1; i < nlk; ++i) per_cu = std::min(per_cu, blocks_per_cu(h->cfg.device_id, lk[i]));
    // One wave per chain at d > 20 (window_kernel_pw, or the program's own): ONE workgroup per CU (its registers, from d = 23 on
    // its LDS too: 86-111 KB).  A launch of 1024 chains is then a workgroup on every CU, and what else runs on the chip beside
    // it (producer workgroups, the R-hat kernels: finite, they wait for nothing) can delay a consumer workgroup's start but not
    // prevent it -- the same argument as for the regression kernel's full-LDS workgroups below.  No halving there (undone by
    // the doubling).
    if (h->split_kind == SPLIT_WAVE && h->cfg.d > 20 && per_cu == 1) per_cu = 2;
    // window_kernel_lr8s: every consumer workgroup takes a CU's LDS for itself (the design matrix): the launch's 256 workgroups are
    // resident together iff every CU is there for them, and a CU's other tenants (producer workgroups of the same grid come behind
    // the consumers and need the same LDS; the R-hat kernels need none) cannot take it from them.  No halving here either.
    if (h->lr_spec) per_cu *= 2;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device_id) != hipSuccess) cus = 0;
    h->live_wg_cap = (int64_t)per_cu * cus / 2;
    return h->live_wg_cap;
}

// Generations one LIVE launch of the split layout may span (0: not applicable -- other layouts, sharded
// runs, deferred visibility, appends owned by the caller, more consumer workgroups than may wait for each
// other).  Bounded by the draw records it needs.
// The waves of a LIVE launch wait for each other, so the residency rule above must hold for everything the
// process has in flight on the device: ONE handle per device uses LIVE launches at a time (the first to ask keeps
// the slot until it is destroyed); other handles on that device run one launch per K-window -- same results.
// (Another PROCESS on the GPU is outside this rule; the bounded poll + the automatic redo in demcz_run_checked /
//  check_live_err cover it.)
static std::mutex g_live_mutex;
static int64_t g_live_used[64] = {0};      // per-mille of each device's LIVE capacity held by handles of this process

// Round 4: a budget instead of one owner per device.  A handle claims the share of ITS kernel's capacity that its consumer
// workgroups are (capacities differ by kernel: registers, LDS); claims of a device add up to at most the whole.  That is what
// lets the R replicas of a sharded run share one GPU (demcz_peer_group), each with 1/R of the chains, and lets two small
// independent samplers both keep their LIVE launches.
static bool live_claim(demcz_handle* h)
{
    if (h->live_claimed) return true;
    const int dev = h->cfg.device_id;
    if (dev < 0 || dev >= 64) return false;
    const int64_t cap = live_wg_capacity(h);
    const int64_t wgs = (h->cfg.N + h->split_per_wg - 1) / h->split_per_wg;
    if (cap <= 0 || wgs > cap) return false;
    const int64_t share = std::max<int64_t>(1, (wgs * 1000 + cap - 1) / cap);
    std::lock_guard<std::mutex> lk(g_live_mutex);
    if (g_live_used[dev] + share > 1000) return false;
    g_live_used[dev] += share;
    h->live_share = share;
    h->live_claimed = true;
    return true;
}

static void live_release(demcz_handle* h)
{
    if (!h->live_claimed) return;
    std::lock_guard<std::mutex> lk(g_live_mutex);
    const int dev = h->cfg.device_id;
    if (dev >= 0 && dev < 64) g_live_used[dev] = std::max<int64_t>(0, g_live_used[dev] - h->live_share);
    h->live_share = 0;
    h->live_claimed = false;
}

// A handle that becomes a peer gives up the two-chains-to-a-wave form (window_kernel_ps2d).  That form only takes REGULAR
// launches; its irregular ones (a start or a tail that is not a multiple of five, temperatures outside the arena, a history of
// 4 GiB or more) run the general kernel with one chain per wave -- twice the waves, which are not all resident, so never LIVE --
// and a non-LIVE launch appends N rows per boundary at M_append + b * N: it knows nothing of `brows` / `row_off`, publishes
// nothing to the peers and waits for nothing of theirs, while the host advances M by N * shards (the replicas'
// archives would silently hold sentinel rows read as data).  With one chain per wave every launch of a peer is either LIVE or --
// when the shard's chains are more than a LIVE launch holds (N > 1024 per shard at d <= 5) -- the handle runs the exchange path
// (RCCL all-gather; a replica group: lockstep), which appends all shards' rows itself.  Same results either way.
static void peer_no_dual(demcz_handle* h)
{
    if (!h->ps_dual) return;
    live_release(h);
    h->ps_dual = false;
    h->dual_now = false;
    h->split_per_wg = PS_CHAINS;
    h->live_wg_cap = -1;
    rec_invalidate(h);
}

// layouts whose LIVE consumers re-read a missing row through live_reload (system scope when there are peers)
static bool peer_capable(const demcz_handle* h)
{
    return h->lanes == DEMCZ_LAYOUT_SPLIT && h->split_kind != SPLIT_PC8 && h->split_kind != SPLIT_NONE;
}

// DEMCZ_REC_MIB: MiB of draw records per buffer instead of the built-in choice (measurements)
static int64_t rec_env_mib()
{
    static const int64_t env_mib = getenv("DEMCZ_REC_MIB") ? atol(getenv("DEMCZ_REC_MIB")) : 0;
    return env_mib;
}

static int64_t rec_target_bytes(bool dual)
{
    const int64_t mib = rec_env_mib() > 0 ? rec_env_mib() : (dual ? 2 * ARENA_REC_MIB : ARENA_REC_MIB);
    return mib << 20;
}

static int64_t live_span(demcz_handle* h)
{
    // (sharded: only with the rows handed over inside the launches -- peer_mode 2; otherwise a launch ends at the exchange)
    if (h->lanes != DEMCZ_LAYOUT_SPLIT || (h->comm && h->peer_mode != 2) || h->lag > 0 || h->external_append || h->no_live) return 0;
    if (h->peer_mode != 0 && !peer_capable(h)) return 0;
    if (h->peer_mode == 1 && (!h->group || h->group->failed || h->group->dead)) return 0;
    static const bool disabled = (getenv("DEMCZ_NO_LIVE") != nullptr);     // safety valve: one launch per K-window
    if (disabled) return 0;
    const int per_wg = h->split_per_wg;
    if ((h->cfg.N + per_wg - 1) / per_wg > live_wg_capacity(h)) return 0;
    if (!live_claim(h)) return 0;
    const int64_t per_gen = rec_fields(h) * h->cfg.N * (int64_t)sizeof(double);
    // Inside the arena: what demcz_create sized its buffers for (arena_span, demcz_slab_plan.h: 64 MiB per buffer, C2 1170
    // generations -- longer launches are not faster there, profiles/r10_launch_span.txt).  Outside it 1 GiB of records per buffer (C4's
    // shard 5960 generations instead of 372, C5 5450 instead of 340, C3 820 instead of 51; allocated as launches need it): every
    // launch boundary costs 15-25 us of gap, first-pass latency and tail imbalance -- C4's shard 7.4 -> 6.1 us per K-window,
    // C5 22.3 -> 21.5 (profiles/r03f_launch_span.txt)
    if (h->arena) return std::max<int64_t>(h->cfg.K, std::min<int64_t>(h->arena_span, SPAN_GENS_MAX));
    const int64_t env_mib = rec_env_mib();
    // (block updates, SPLIT_MLB: flat between 64 and 256 MiB, 4 % slower at 1 GiB -- 128)
    const int64_t mib = env_mib > 0 ? env_mib : (h->split_kind == SPLIT_MLB) ? 128 : 1024;
    const int64_t span = (int64_t)(mib << 20) / per_gen;
    return std::max<int64_t>(h->cfg.K, std::min<int64_t>(span, 1 << 20));
}

// Streamed history: generations g_from..g_to (already enqueued on the compute stream) are copied to the pinned host mirrors on
// the copy stream, behind an event -- while the compute stream goes on with the next slab.
static int32_t stream_history(demcz_handle* h, int64_t g_from, int64_t g_to)
{
    if (!h->hs_on || h->cfg.Gcap <= 0 || g_to < g_from) return DEMCZ_OK;
    const int64_t N = h->cfg.N, s0 = g_from - h->g0 - 1, G = g_to - g_from + 1;
    const int d = h->cfg.d;
    if (s0 < 0 || s0 + G > h->cfg.Gcap) return DEMCZ_OK;
    hipEvent_t ev = h->after_launch_ev;
    if (!ev) {
        if (!h->diag_ev) HIPCHK(h, hipEventCreateWithFlags(&h->diag_ev, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(h->diag_ev, h->stream));
        h->after_launch_ev = ev = h->diag_ev;
    }
    HIPCHK(h, hipStreamWaitEvent(h->hs_stream, ev, 0));
    HIPCHK(h, hipMemcpyAsync(h->hs_chain + (size_t)N * d * s0, h->dchain + (size_t)N * d * s0, (size_t)N * d * G * sizeof(double), hipMemcpyDeviceToHost, h->hs_stream));
    HIPCHK(h, hipMemcpyAsync(h->hs_logobj + (size_t)N * s0, h->dlogobj + (size_t)N * s0, (size_t)N * G * sizeof(double), hipMemcpyDeviceToHost, h->hs_stream));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_history_stream(demcz_handle* h, int32_t enabled)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (h->cfg.Gcap <= 0) return fail(h, DEMCZ_ERR_STATE, "demcz_history_stream: handle keeps no history (Gcap = 0)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (enabled && !h->hs_on) {
        const size_t nc = (size_t)h->cfg.N * h->cfg.d * h->cfg.Gcap * sizeof(double), nl = (size_t)h->cfg.N * h->cfg.Gcap * sizeof(double);
        if (!h->hs_chain) HIPCHK(h, g_host_pool.acquire((void**)&h->hs_chain, nc, -1));
        if (!h->hs_logobj) HIPCHK(h, g_host_pool.acquire((void**)&h->hs_logobj, nl, -1));
        if (!h->hs_stream) HIPCHK(h, stream_acquire(h->cfg.device_id, &h->hs_stream));
    }
    h->hs_on = enabled != 0;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_history_view(demcz_handle* h, int64_t g_from, int64_t g_to, double** chain, double** log_obj)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_get_history_view");
    if (rc) return rc;
    if (!h->hs_on || !h->hs_chain) return fail(h, DEMCZ_ERR_STATE, "demcz_get_history_view: call demcz_history_stream(h, 1) before the run");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = live_verify(h);                       // (a voided LIVE slab is redone here, and the redo streams its generations again)
    if (rc) return rc;
    rc = sync_stream(h, h->hs_stream, "demcz_get_history_view");
    if (rc) return rc;
    const int64_t s0 = g_from - h->g0 - 1;
    if (chain) *chain = h->hs_chain + (size_t)h->cfg.N * h->cfg.d * s0;
    if (log_obj) *log_obj = h->hs_logobj + (size_t)h->cfg.N * s0;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_detach_history(demcz_handle* h, void** chain_base, void** logobj_base)
{
    NOT_DERIVED(h);
    if (!h || !chain_base || !logobj_base) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->hs_chain) return fail(h, DEMCZ_ERR_STATE, "demcz_detach_history: no streamed history on this handle");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (h->hs_stream) { int32_t rc = sync_stream(h, h->hs_stream, "demcz_detach_history"); if (rc) return rc; }
    *chain_base = h->hs_chain; *logobj_base = h->hs_logobj;
    h->hs_chain = h->hs_logobj = nullptr;      // the caller owns them now: demcz_release_host_buffer
    h->hs_on = false;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_release_host_buffer(void* base)
{
    if (base) g_host_pool.release(base, -1);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_pool_trim(int64_t* device_bytes, int64_t* pinned_bytes)
{
    const size_t a = g_dev_pool.trim(), b = g_host_pool.trim();
    if (device_bytes) *device_bytes = (int64_t)a;
    if (pinned_bytes) *pinned_bytes = (int64_t)b;
    return DEMCZ_OK;
}

// what a caller that makes several calls in a row knows beyond the call at hand (demcz_run_checked)
struct RunHints {
    int32_t bracket_slabs = 1;        // autostop slabs the call covers (kernel timing: one event bracket per call)
    int64_t next_ngen = 0;            // generations of the launch that follows the call (0: not known)
};

// a call that is to be made (a replica group without its hand-off) or made again (a failed LIVE hand-off)
static void log_run_call(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature)
{
    demcz_handle::RunCall rcall{g_from, g_to, gamma, temperature != nullptr, {}};
    if (temperature) rcall.temperature.assign(temperature, temperature + (g_to - g_from + 1));
    h->live_log.push_back(std::move(rcall));
}

// cr_adapt_kernel on the handle's stream: the update of the class weights with the spread (d + 1 workgroups), or the spread alone
static int32_t launch_cr_adapt(demcz_handle* h, bool update)
{
    CrAdaptUpdate U{};
    U.X = h->dX; U.N = h->cfg.N; U.d = h->cfg.d; U.ncr = h->cr_ncr; U.min_weight = h->cr_adapt_min_weight;
    U.nwg = (int32_t)cra_workgroups(h);
    U.weights = reinterpret_cast<int32_t*>(h->d_cr_adapt + CRA_WEIGHTS);
    U.cum = reinterpret_cast<uint32_t*>(h->d_cr_adapt + CRA_CUM);
    U.updates = reinterpret_cast<long long*>(h->d_cr_adapt + CRA_UPDATES);
    U.rsd = reinterpret_cast<double*>(h->d_cr_adapt + CRA_RSD);
    U.slots = reinterpret_cast<unsigned long long*>(h->d_cr_adapt + CRA_SLOTS);
    void* args[] = {&U};
    HIPCHK(h, hipLaunchKernel(crossover_adapt_update_fn(), dim3((unsigned)(h->cfg.d + (update ? 1 : 0))), dim3(64), args, 0, h->stream));
    HIPCHK(h, hipGetLastError());
    return DEMCZ_OK;
}

// demcz_run.  The schedule -- where each window launch ends and of what kind it is -- is plan_launch's (demcz_run_plan.h); this is
// its executor.
static int32_t run_call(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature, const RunHints& hints)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_run: call demcz_set_state first");
    if (g_from < 1 || g_to < g_from) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_run: need 1 <= g_from <= g_to");
    if (h->cfg.target_kind == DEMCZ_TARGET_HOST_CALLBACK)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: host-callback target uses demcz_propose/accept_commit");
    const bool hist = h->cfg.Gcap > 0;
    if (hist && (g_from - h->g0 - 1 < 0 || g_to - h->g0 > h->cfg.Gcap))
        return fail(h, DEMCZ_ERR_CAPACITY, "demcz_run: generations outside the history window (demcz_set_history_origin)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int64_t G = g_to - g_from + 1;
    const int K = h->cfg.K;
    const bool sharded = (h->comm != nullptr);
    if (h->peer_mode == 1 && (!h->group || h->group->dead))
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: a member of this handle's replica group has been destroyed");
    if (h->no_live && h->rearm_from >= 0 && g_from > h->rearm_from) {
        // behind the generation a hand-off failed at: LIVE launches again (the calls up to here ran one launch per K-window)
        int32_t rcr = live_try_rearm(h);
        if (rcr) return rcr;
    }
    // `peer`: the boundary rows of ALL shards reach this replica from inside the launches (live_publish) -- no exchange step
    const bool peer = h->peer_mode != 0 && live_span(h) > 0;
    const bool rccl_exchange = sharded && !peer;
    const bool kernel_appends = !rccl_exchange && !h->external_append;
    const int64_t shards = (sharded || h->peer_mode != 0) ? h->nranks : 1;
    // capacity check for all appends of this call
    {
        const int64_t nb = boundaries_in(g_from, g_to, K);
        const int64_t rows = h->cfg.N * shards;
        if (!h->external_append && h->M_app + nb * rows > h->cfg.Mcap)
            return fail(h, DEMCZ_ERR_CAPACITY, "demcz_run: Z row capacity (Mcap) would be exceeded");
        if (h->external_append && nb > 1)
            return fail(h, DEMCZ_ERR_STATE, "demcz_run: with external append a call may cross at most one K boundary, at its end");
        if (h->external_append && nb == 1 && (g_to % K) != 0)
            return fail(h, DEMCZ_ERR_STATE, "demcz_run: with external append the K boundary must be the last generation of the call");
    }
    if (h->cr_ncr > 0 && h->M < 2)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: crossover generations draw pairs of distinct archive rows: the archive has fewer than two "
                                        "(demcz_set_crossover with ncr = 0 switches them off)");
    if (h->snooker_every > 0 && h->M < 3)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: snooker generations draw three distinct archive rows: the archive has fewer than three "
                                        "(demcz_set_snooker with every = 0 switches them off)");
    if (h->peer_mode == 3 && h->peers_closed)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: the peers' archives have been closed (demcz_peer_detach): this handle runs no further generations");
    if (h->peer_mode == 3 && !peer)
        return fail(h, DEMCZ_ERR_STATE, "demcz_run: host-mediated IPC peers run with the in-launch hand-off only (it is not available: a timed-out "
                                        "hand-off, an append lag, caller-owned appends, or more chains than a LIVE launch holds)");
    if (h->peer_mode == 1 && !peer && !h->replaying) {
        // A replica group that lost (or never had) its in-launch hand-off: its members cannot exchange rows by themselves, so
        // the call is only logged here and executed for ALL members in lockstep, one launch per K-window, at the next
        // verification (group_verify) -- by which time every member has been given the same call.
        if (h->lag != 0 || h->external_append) return fail(h, DEMCZ_ERR_STATE, "demcz_run: replica groups run with append lag 0 and library-owned appends");
        log_run_call(h, g_from, g_to, gamma, temperature);
        return DEMCZ_OK;
    }
    // (a handle with the arena keeps a call's temperatures inside it when they fit: window_kernel_ps2 then reaches them with the
    //  32-bit offsets it reaches everything else with)
    const bool temp_in_arena = temperature && h->arena && h->arena_temp && G <= h->arena_gens;
    if (temperature && temp_in_arena) {
        SYNCCHK_AS(h, h->stream, "demcz_run");              // (earlier windows may still read the region)
        HIPCHK(h, hipMemcpyAsync(h->arena_temp, temperature, (size_t)G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        SYNCCHK_AS(h, h->stream, "demcz_run");              // the caller may reuse its buffer on return
    } else if (temperature) {
        if (G > h->temp_cap) {
            { int32_t rcq = quiesce_all(h); if (rcq) return rcq; }
            SYNCCHK_AS(h, h->stream, "demcz_run");
            if (h->dtemp) HIPCHK(h, dev_free(h->cfg.device_id, h->dtemp));
            h->dtemp = nullptr; h->temp_cap = 0;
            // (+ 8: the wave-per-chain consumer fetches a pass's temperatures as whole 16-byte pieces, demcz_kernels_ps.h)
            HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->dtemp, (size_t)(G + 8) * sizeof(double)));
            HIPCHK(h, hipMemsetAsync(h->dtemp, 0, (size_t)(G + 8) * sizeof(double), h->stream));
            h->temp_cap = G;
        }
        // stream-ordered behind earlier windows that still read dtemp
        HIPCHK(h, hipMemcpyAsync(h->dtemp, temperature, (size_t)G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        SYNCCHK_AS(h, h->stream, "demcz_run");   // the caller may reuse its buffer on return
    }
    WindowParams P;
    P.Z = h->dZ; P.Zw = h->dZ; P.ZS = h->ZS;
    P.Xcur = h->dX; P.lpcur = h->dlp;
    P.chain = hist ? h->dchain : nullptr; P.logobj = hist ? h->dlogobj : nullptr;
#ifdef DEMCZ_EXP_NOHIST           // (timing experiment, never the shipped library: no window kernel writes any history --
    P.chain = nullptr; P.logobj = nullptr;      //  scripts/build_variant.py nohist -DDEMCZ_EXP_NOHIST; profiles/r04o_history_store.txt)
#endif
    P.N = h->cfg.N; P.chain_id0 = h->cfg.chain_id0; P.d = h->cfg.d;
    P.gamma = gamma; P.seed = h->cfg.seed; P.S = h->S; P.Nblocks = h->cfg.Nblocks;
    P.block_offsets = h->d_block_offsets; P.slot_of = h->d_slot_of; P.eps = h->d_eps; P.slot_role = h->d_slot_role;
    P.tp = target_params(h);
    P.snap = nullptr;
    P.K = K;
    P.acc_out = nullptr; P.live_err = h->d_live_err; P.live_spin_limit = LIVE_SPIN_LIMIT;
    P.safe_X = nullptr; P.safe_lp = nullptr;
    P.rec_in = nullptr; P.rec_out = nullptr; P.next_g_first = 0; P.next_M = 0; P.next_ngen = 0; P.consumer_blocks = 0;
    P.next_rows = 0; P.next_boff = 0; P.rec_stride = 0;
    P.rec_fields = (h->lanes == DEMCZ_LAYOUT_SPLIT && h->split_kind == SPLIT_ML) ? h->cfg.d + 2 : 0;    // lane-per-parameter consumers: record-major
    P.z_bytes = (uint32_t)std::min<size_t>(h->dZ_bytes, 0xffffffffull);
    P.hist_bytes = (hist && h->hist_joint) ? hist_bytes_u32(h->cfg.N, h->cfg.d, h->cfg.Gcap) : 0u;
    P.brows = h->cfg.N * (peer ? shards : 1);
    P.row_off = peer ? (int64_t)h->rank * h->cfg.N : 0;
    P.n_peers = peer ? h->n_peers : 0;
    for (int r = 0; r < DEMCZ_MAX_PEERS; ++r) P.peer_Z[r] = (peer && r < h->n_peers) ? h->peer_Z[r] : nullptr;
    if (peer && h->peer_mode == 2 && h->peer_fence) {
        // this replica's unwritten rows were re-filled with the sentinel (set_state / a rollback) on this stream: no peer may
        // publish into it before that is done, so the ranks meet here, stream-ordered, before the first launch that publishes
        NCCLCHK(h, ncclAllReduce(h->d_err_all + 1, h->d_err_all + 1, 1, ncclUint32, ncclMax, h->comm, h->stream));
        h->peer_fence = false;
    }
#ifdef DEMCZ_STAMPS
    if (!h->d_stamps) {
        HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_stamps, (size_t)DEMCZ_STAMP_WGS * 16 * sizeof(unsigned long long)));
        HIPCHK(h, hipMemset(h->d_stamps, 0, (size_t)DEMCZ_STAMP_WGS * 16 * sizeof(unsigned long long)));
    }
    P.stamps = h->d_stamps;
#endif
    const int E = h->lag;
    if (h->lanes == DEMCZ_LAYOUT_SPLIT) {
        // draw-record buffers: sized ONCE for the longest launch this handle can make -- a LIVE launch spans up
        // to live_span() generations (never more than the run is long: Gcap, when a history is kept), any other
        // at most a K-window / a batch of E windows -- before anything of this call is timed or enqueued
        const int64_t lm = live_span(h);
        int64_t cap = (lm > 0) ? lm : (int64_t)K * std::max(E, 1);
        if (lm > 0 && hist) cap = std::max<int64_t>(std::min<int64_t>(cap, h->cfg.Gcap), std::min<int64_t>(cap, G));
        int32_t rcr = rec_reserve(h, cap);
        if (rcr) return rcr;
    }
    if (live_span(h) > 0) {
        // this call may issue LIVE launches: they are verified at the next synchronising entry point, and redone
        // from here (live_verify) should a row hand-off inside one of them fail
        // bound the redo: verify now (a synchronisation every 256 calls).  Not inside demcz_run_checked: that call rolls back
        // to ITS entry and redoes itself from there (statistics and stop decisions included), so the snapshot must not move
        // into the middle of it.  Not inside a redo either (`replaying`): a call of a redo that has re-armed is logged against
        // the verified point the redo started from -- the snapshot taken there is the one a second failure goes back to.
        if (h->live_log.size() >= 256 && !h->in_checked && !h->replaying && h->peer_mode != 1) {      // (a replica group verifies as a whole: group_verify)
            int32_t rcv = live_verify(h);
            if (rcv) return rcv;
        }
        if (live_span(h) > 0) {
            if (h->live_log.empty() && !h->replaying) {
                const int64_t N = h->cfg.N;
                const int d = h->cfg.d;
                if (!h->d_safe_X) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_safe_X, (size_t)N * d * sizeof(double)));
                if (!h->d_safe_lp) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_safe_lp, (size_t)N * sizeof(double)));
                if (h->live_fault_polls < 0) {   // fault injection: whatever the snapshot buffers held must never reach the state
                    HIPCHK(h, hipMemsetAsync(h->d_safe_X, 0xff, (size_t)N * d * sizeof(double), h->stream));
                    HIPCHK(h, hipMemsetAsync(h->d_safe_lp, 0xff, (size_t)N * sizeof(double), h->stream));
                }
                h->snap_pending = true;          // (made by the first launch: launch_window)
                h->safe_M = h->M; h->safe_M_app = h->M_app; h->safe_g_done = h->g_done;
            }
            log_run_call(h, g_from, g_to, gamma, temperature);
        }
    }
    // demcz_set_kernel_timing: ONE event pair around the back-to-back window launches of this call (an event
    // between two launches would put a bubble into the stream it is meant to measure)
    struct EventPair {          // destroyed on every error return; handed to h->timed on success
        hipEvent_t a = nullptr, b = nullptr;
        ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } tev;
    int64_t timed_launches = 0;
    const bool timed = h->timing && h->timed.size() < 4096;
    if (timed) {
        HIPCHK(h, hipEventCreate(&tev.a));
        HIPCHK(h, hipEventCreate(&tev.b));
        HIPCHK(h, hipEventRecord(tev.a, h->stream));
    }
    // what the schedule of this call rests on (plan_launch, demcz_run_plan.h)
    RunFacts F;
    F.K = K; F.E = E; F.external_append = h->external_append;
    F.N = h->cfg.N; F.shards = shards; F.peer = peer;
    F.g_to = g_to; F.G = G; F.rng_offset = h->rng_offset;
    F.split = h->lanes == DEMCZ_LAYOUT_SPLIT; F.hist = hist;
    F.two_chain = h->ps_dual; F.R = PS2_R;
    F.temp_in_arena = !temperature || temp_in_arena;
    F.hist_32bit = hist_offsets_32bit(h->cfg.N, h->cfg.d, h->cfg.Gcap);
    F.arena = h->arena;
    F.cold_limit = cold_start_limit(K, rec_fields(h) * h->cfg.N * (int64_t)sizeof(double), h->ps_dual);
    F.next_hint = hints.next_ngen;
    // (DEMCZ_FORCE_LIVE_KERNEL=1, diagnosis only: the LIVE instantiation also for launches with no boundary inside -- what the
    //  instantiation itself costs, scripts/live_fixed_cost.py)
    static const bool force_live = getenv("DEMCZ_FORCE_LIVE_KERNEL") != nullptr;
    F.force_live = force_live;
    F.snooker_every = h->snooker_every;
    F.adapt_every = h->cr_adapt_every;
    F.adapt_until = h->cr_adapt_until;
    if (h->cr_adapt_every > 0 && !h->cr_adapt_started) {
        // the start of adaptation: the spread of the chains as they stand (no restored state)
        int32_t rca = launch_cr_adapt(h, false);
        if (rca) return rca;
        h->cr_adapt_started = true;
    }
    for (int64_t g = g_from; g <= g_to;) {
        F.rec_in_arena = h->rec_in_arena;         // (pc_prepare moves the buffers out of the arena should a caller outrun what was reserved)
        const LaunchPlan lp = plan_launch(F, g, live_span(h), h->M, h->M_app, h->rec_desc[h->rec_cur], h->pending);
        const int64_t w_end = lp.w_end, nbound = lp.nbound;
        h->dual_now = lp.dual;
        h->snooker_now = lp.snooker;
        h->cr_accumulate_now = adapt_accumulates(F, g);
        int32_t rc = admit_pending(h, g);
        if (rc) return rc;
        P.M = h->M;
        P.M_append = h->M_app;
        P.g_first = g + h->rng_offset;      // only positions the Philox streams
        P.ngen = (int32_t)(w_end - g + 1);
        P.to_boundary = (int32_t)lp.to_boundary;
        P.slot_first = hist ? (g - h->g0 - 1) : 0;
        P.temperature = temperature ? (temp_in_arena ? h->arena_temp : h->dtemp) + (g - g_from) : nullptr;
        P.do_append = (nbound > 0 && kernel_appends) ? 1 : 0;
        P.snap = nullptr;
        if (nbound > 0 && rccl_exchange && E > 0) {
            if (h->batch_cnt == 0) {
                // the buffer was last read by the exchange two batches ago
                // (every wait is a barrier packet between two window kernels: not asked for twice)
                if (h->buf_xseq[h->batch_buf] > h->xseq_waited) HIPCHK(h, hipStreamWaitEvent(h->stream, h->buf_done[h->batch_buf], 0));
                h->batch_base = h->M_app;
            }
            P.snap = h->d_send[h->batch_buf] + (size_t)h->batch_cnt * h->cfg.N * h->cfg.d;
        }
        if (F.split) {
            rc = pc_prepare(h, P, lp);
            if (rc) return rc;
        }
        const bool live = lp.live;
        P.live_err = h->d_live_err;
        P.live_spin_limit = h->live_spin_limit ? (int32_t)h->live_spin_limit : LIVE_SPIN_LIMIT;
        if (h->live_fault_polls > 0 && g >= h->live_fault_g) P.live_spin_limit = h->live_fault_polls;
        if (h->live_fault_polls < 0 && live && g >= h->live_fault_g)      // "a wave of this launch has already given up": every wave leaves at once
            HIPCHK(h, hipMemsetAsync(h->d_live_err, 0x01, sizeof(unsigned int), h->stream));
        P.acc_out = h->d_acc ? h->d_acc + (size_t)h->acc_next * (size_t)h->acc_waves * 2 : nullptr;
        if (h->ps_dual && P.acc_out)     // (its two kernels write different numbers of waves' counters into a slot of the ring)
            HIPCHK(h, hipMemsetAsync(P.acc_out, 0, (size_t)h->acc_waves * 2 * sizeof(unsigned int), h->stream));
        if (live) h->err_clean = false;
        rc = launch_window(h, P, live);
        h->snooker_now = false;
        h->after_launch_ev = nullptr;         // (whatever was recorded before this launch says nothing about it)
        if (rc) return rc;
        if (lp.snooker) ++h->snooker_steps;
        // the launch ended on an update position: the new weights and the spread, stream-ordered behind it and in front of the next
        if (lp.adapt_after) { rc = launch_cr_adapt(h, true); if (rc) return rc; }
        if (h->d_acc) {
            h->acc_log.push_back({g, w_end, h->acc_next});
            h->acc_next = (h->acc_next + 1) % h->acc_slots;
            if ((int64_t)h->acc_log.size() > h->acc_slots) h->acc_log.pop_front();
        }
        ++timed_launches;
        // streamed history: this launch's generations leave for the host mirrors behind it, while the next launch computes
        // (one marker per launch on the compute stream: launches that stream are long ones)
        if (h->hs_on && hist) { int32_t rch = stream_history(h, g, w_end); if (rch) return rch; }
        if (nbound > 0 && !h->external_append) {
            const int64_t rows = h->cfg.N * shards;
            if (E == 0) {
                if (kernel_appends) { h->M_app += nbound * rows; h->M = h->M_app; }
                else { rc = append_after_window(h); if (rc) return rc; }
            } else {
                for (int64_t j = (g - 1) / K + 1; j <= w_end / K; ++j) {
                    const int64_t J = lag_batch_of(j, E);
                    h->M_app += rows;
                    if (h->batch_J != J) {
                        h->pending.push_back({lag_visible_from(J, E, K), h->M_app, nullptr});
                        h->batch_J = J;
                    } else {
                        h->pending.back().M_after = h->M_app;
                    }
                    if (rccl_exchange) {
                        ++h->batch_cnt;
                        if (j == J) { rc = exchange_batch(h); if (rc) return rc; }
                    }
                }
            }
        }
        g = w_end + 1;
    }
    if (timed) {
        HIPCHK(h, hipEventRecord(tev.b, h->stream));
        h->after_launch_ev = tev.b;
        h->timed.emplace_back(tev.a, tev.b);
        h->timed_slabs.push_back(std::max(hints.bracket_slabs, 1));
        tev.a = tev.b = nullptr;
        h->timed_launches += timed_launches;
    }
    if (rccl_exchange && E > 0) {           // nothing stays un-exchanged across calls
        int32_t rc = exchange_batch(h);
        if (rc) return rc;
    }
    h->g_done = g_to;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_run(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature)
{
    NOT_DERIVED(h);
    return run_call(h, g_from, g_to, gamma, temperature, RunHints{});
}

extern "C" int32_t demcz_synchronize(demcz_handle* h)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    SYNCCHK(h, h->stream);
    if (h->comm_stream) SYNCCHK(h, h->comm_stream);
    if (h->prod_stream) SYNCCHK(h, h->prod_stream);      // (the next launch's draws, monitoring checks)
    return live_verify(h);
}

static int32_t check_hist_range(demcz_handle* h, int64_t g_from, int64_t g_to, const char* who)
{
    if (h->cfg.Gcap <= 0) return fail(h, DEMCZ_ERR_STATE, std::string(who) + ": handle keeps no history (Gcap = 0)");
    if (g_from < 1 || g_to < g_from || g_from - h->g0 - 1 < 0 || g_to - h->g0 > h->cfg.Gcap)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": generations outside the history window");
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_history(demcz_handle* h, int64_t g_from, int64_t g_to, double* chain, double* log_obj)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (log_obj) NOT_DERIVED(h);               // (a derived history has values only)
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_get_history");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = live_verify(h);
    if (rc) return rc;
    const int64_t N = h->cfg.N, G = g_to - g_from + 1, s0 = g_from - h->g0 - 1;
    const int d = h->cfg.d;
    if (chain)
        HIPCHK(h, hipMemcpyAsync(chain, h->dchain + (size_t)N * d * s0, (size_t)N * d * G * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    if (log_obj)
        HIPCHK(h, hipMemcpyAsync(log_obj, h->dlogobj + (size_t)N * s0, (size_t)N * G * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_changed(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t* changed)
{
    NOT_DERIVED(h);
    if (!h || !changed) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_get_changed");
    if (rc) return rc;
    const int64_t G = g_to - g_from + 1, s0 = g_from - h->g0 - 1;
    if (s0 == 0 && !h->origin_valid)
        return fail(h, DEMCZ_ERR_STATE, "demcz_get_changed: the log_obj before the first history slot is not known "
                                        "(set the history origin when exactly g0 generations have been run)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = live_verify(h);
    if (rc) return rc;
    rc = ensure_scratch(h, G);
    if (rc) return rc;
    static_assert(sizeof(long long) == sizeof(double), "scratch reuse");
    hipLaunchKernelGGL(changed_from_history_kernel, dim3((unsigned)G), dim3(256), 0, h->stream, (const double*)h->dlogobj,
                       (const double*)h->dlp_origin, h->cfg.N, s0, (long long*)h->d_scratch);
    HIPCHK(h, hipGetLastError());
    static_assert(sizeof(int64_t) == sizeof(long long), "int64 layout");
    HIPCHK(h, hipMemcpyAsync(changed, h->d_scratch, (size_t)G * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

namespace demcz {
// sum over `nslots` consecutive ring slots (from slot0, modulo `ring`) of the per-wave launch totals, minus the
// first-generation counts of slot0 when `skip_first`
__global__ void __launch_bounds__(256) sum_counts_kernel(const unsigned int* acc, int64_t waves, int slot0, int nslots, int ring,
                                                         int skip_first, long long* out)
{
    __shared__ long long red[256];
    long long a = 0;
    for (int64_t i = threadIdx.x; i < (int64_t)nslots * waves; i += 256) {
        const int sl = (int)(i / waves);
        const int64_t w = i % waves;
        const unsigned int* e = acc + ((size_t)((slot0 + sl) % ring) * (size_t)waves + (size_t)w) * 2;
        a += (long long)e[0];
        if (skip_first && sl == 0) a -= (long long)e[1];
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}
}  // namespace demcz

extern "C" int32_t demcz_get_changed_total(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t* total, int32_t* from_ballots)
{
    NOT_DERIVED(h);
    if (!h || !total || g_from < 1 || g_to < g_from) return DEMCZ_ERR_INVALID_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rc = live_verify(h);
    if (rc) return rc;
    // whole launches whose generations are exactly g_from..g_to, or g_from-1..g_to with the first generation's own
    // count taken off (the window sum of demcz_anneal.jl:50 has no predecessor for its first column)
    int first = -1, last = -1, skip = 0;
    for (int i = 0; i < (int)h->acc_log.size(); ++i) {
        const auto& r = h->acc_log[i];
        if (first < 0 && (r.g_first == g_from || r.g_first == g_from - 1) && r.g_last >= g_from) { first = i; skip = (r.g_first == g_from - 1); }
        if (first >= 0 && r.g_last == g_to) { last = i; break; }
    }
    bool ok = first >= 0 && last >= first;
    for (int i = first; ok && i < last; ++i)
        ok = h->acc_log[i].g_last + 1 == h->acc_log[i + 1].g_first && (h->acc_log[i].slot + 1) % h->acc_slots == h->acc_log[i + 1].slot;
    if (ok && h->d_acc) {
        rc = ensure_scratch(h, 1);
        if (rc) return rc;
        static_assert(sizeof(long long) == sizeof(double), "scratch reuse");
        hipLaunchKernelGGL(sum_counts_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned int*)h->d_acc, h->acc_waves,
                           (int)h->acc_log[first].slot, last - first + 1, (int)h->acc_slots, skip, (long long*)h->d_scratch);
        HIPCHK(h, hipGetLastError());
        long long v = 0;
        HIPCHK(h, hipMemcpyAsync(&v, h->d_scratch, sizeof(v), hipMemcpyDeviceToHost, h->stream));
        SYNCCHK(h, h->stream);
        *total = (int64_t)v;
        if (from_ballots) *from_ballots = 1;
        return DEMCZ_OK;
    }
    // not a union of whole launches (or a host-closure handle): count from the history, as the checker does
    std::vector<int64_t> ch((size_t)(g_to - g_from + 1));
    rc = demcz_get_changed(h, g_from, g_to, ch.data());
    if (rc) return rc;
    int64_t t = 0;
    for (int64_t v : ch) t += v;
    *total = t;
    if (from_ballots) *from_ballots = 0;
    return DEMCZ_OK;
}

// ---- R-hat ---------------------------------------------------------------------------------------
// (slabs > 1: a batch of checks over consecutive windows of w generations, slab z in its own slice of `need` doubles at
//  h->d_scratch + z need; their statistics side by side in `out`, slabs x d doubles behind the last slice)
struct RhatPlan { int64_t N, w, s0, n, nd, need; int d, nchunk; double *S1, *S2, *mean_j, *s2_j, *sums; int slabs = 1; double* out = nullptr; };

// The window's shape and what its plan needs of the scratch buffer (r.need doubles); allocates and launches nothing.
static int rhat_chunks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(1, n / 32), 32); }
static int64_t rhat_need(int64_t nd, int d, int nchunk) { return 2 * (2 * nchunk * nd) + 2 * (2 * nd) + 4 * d; }

static int32_t rhat_plan(demcz_handle* h, int64_t g_from, int64_t g_to, RhatPlan& r, const char* who = "demcz_rhat")
{
    int32_t rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    r.N = h->cfg.N; r.w = g_to - g_from + 1; r.s0 = g_from - h->g0 - 1; r.d = h->cfg.d;
    r.n = r.w / 2;                                            // utils.jl:4
    if (r.n < 2) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": window needs at least 4 generations");
    r.nchunk = rhat_chunks(r.n);
    r.nd = r.N * r.d;
    r.need = rhat_need(r.nd, r.d, r.nchunk);
    return DEMCZ_OK;
}

// The scratch for a plan, with `extra` doubles behind it (at h->d_scratch + r.need) for a statistic that builds on the split
// chains' means, and (compute) the moments and per-chain statistics.
static int32_t rhat_scratch(demcz_handle* h, RhatPlan& r, int64_t extra, bool compute, hipStream_t qs = nullptr)
{
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rc = ensure_scratch(h, r.need * r.slabs + (r.slabs > 1 ? (int64_t)r.slabs * r.d : 0) + extra);
    if (rc) return rc;
    r.S1 = h->d_scratch;
    r.S2 = r.S1 + 2 * r.nchunk * r.nd;
    r.mean_j = r.S2 + 2 * r.nchunk * r.nd;
    r.s2_j = r.mean_j + 2 * r.nd;
    r.sums = r.s2_j + 2 * r.nd;          // [0,d): stage 0 / grand mean; [d,3d): stage 1; [3d,4d): R-hat
    r.out = r.slabs > 1 ? h->d_scratch + r.need * r.slabs : r.sums + 3 * r.d;
    if (compute) {
        const int bs = 256;
        const unsigned gx = (unsigned)((r.nd + bs - 1) / bs);
        if (!qs) qs = h->stream;
        hipLaunchKernelGGL(rhat_moments_kernel, dim3(gx, 2 * r.nchunk, r.slabs), dim3(bs), 0, qs, h->dchain, r.N, r.d, r.s0, r.n, r.nchunk, r.S1, r.S2,
                           r.w, r.need);
        hipLaunchKernelGGL(rhat_chainstats_kernel, dim3(gx, 2, r.slabs), dim3(bs), 0, qs, h->dchain, r.N, r.d, r.s0, r.n, r.nchunk, r.S1, r.S2, r.mean_j,
                           r.s2_j, r.w, r.need);
        HIPCHK(h, hipGetLastError());
    }
    return DEMCZ_OK;
}

static int32_t rhat_prepare(demcz_handle* h, int64_t g_from, int64_t g_to, RhatPlan& r, bool compute, hipStream_t qs = nullptr, int slabs = 1)
{
    int32_t rc = rhat_plan(h, g_from, g_to, r);
    if (rc) return rc;
    if (slabs > 1) {
        rc = check_hist_range(h, g_from, g_from + r.w * slabs - 1, "demcz_run_checked");
        if (rc) return rc;
        r.slabs = slabs;
    }
    return rhat_scratch(h, r, 0, compute, qs);
}

extern "C" int32_t demcz_rhat_partial(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t stage, const double* grand, double* out)
{
    if (!h || !out || (stage != 0 && stage != 1) || (stage == 1 && !grand)) return DEMCZ_ERR_INVALID_ARGUMENT;
    RhatPlan r;
    int32_t rc = live_verify(h);
    if (rc) return rc;
    rc = rhat_prepare(h, g_from, g_to, r, true);
    if (rc) return rc;
    const int d = r.d;
    if (stage == 0) {
        hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, h->stream, r.mean_j, r.s2_j, r.N, d, 0, (const double*)nullptr, 1.0, r.sums);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out, r.sums, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(r.sums, grand, (size_t)d * sizeof(double), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, h->stream, r.mean_j, r.s2_j, r.N, d, 1, (const double*)r.sums, 1.0, r.sums + d);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out, r.sums + d, (size_t)2 * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

// Enqueues the R-hat of generations g_from..g_to and the copy of its d values to `out` (host memory; pinned
// if the caller wants the copy to be asynchronous); does not wait.
// `side`: unsharded runs only -- the statistic of a finished slab is computed on a second stream, behind an event,
// beside the next slab's window kernel (which leaves most of the chip idle at small N).
// `slabs` > 1 (unsharded only): the checks of that many consecutive windows, g_from..g_to the first, as one batch -- three
// launches and one copy of slabs x d doubles to `out`.
static int32_t rhat_enqueue(demcz_handle* h, int64_t g_from, int64_t g_to, double* out, bool side = false, int slabs = 1)
{
    RhatPlan r;
    hipStream_t qs = h->stream;
    // Monitoring checks run beside the next slab.  Where the handle already has a side stream -- the producer stream of the
    // wave-per-chain layout -- they go there, behind the producer kernel: a third active queue cost 10-15 us per
    // 1000-generation slab (the consumer of the next slab started that much later; scripts/step_overhead.py).
    static const bool own_env = getenv("DEMCZ_RHAT_OWN_STREAM") != nullptr;
    if (side && !h->comm && !own_env && h->prod_stream) {
        if (!h->diag_ev) HIPCHK(h, hipEventCreateWithFlags(&h->diag_ev, hipEventDisableTiming));
        if (h->after_launch_ev) {
            HIPCHK(h, hipStreamWaitEvent(h->prod_stream, h->after_launch_ev, 0));
        } else {
            HIPCHK(h, hipEventRecord(h->diag_ev, h->stream));
            HIPCHK(h, hipStreamWaitEvent(h->prod_stream, h->diag_ev, 0));
            h->after_launch_ev = h->diag_ev;
        }
        qs = h->prod_stream;
    } else if (side && h->comm && h->peer_mode == 2 && !h->no_live && h->comm_side && h->comm_stream && h->lag == 0) {
        // sharded with the rows handed over inside the launches: nothing else of this handle uses the side communicator, and the
        // compute stream carries no collective between two slabs -- the statistic goes beside the next slab
        if (!h->diag_ev) HIPCHK(h, hipEventCreateWithFlags(&h->diag_ev, hipEventDisableTiming));
        if (h->after_launch_ev) {
            HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->after_launch_ev, 0));
        } else {
            HIPCHK(h, hipEventRecord(h->diag_ev, h->stream));
            HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->diag_ev, 0));
            h->after_launch_ev = h->diag_ev;
        }
        qs = h->comm_stream;
    } else if (side && !h->comm) {
        if (!h->diag_stream) HIPCHK(h, stream_acquire(h->cfg.device_id, &h->diag_stream));
        if (!h->diag_ev) HIPCHK(h, hipEventCreateWithFlags(&h->diag_ev, hipEventDisableTiming));
        if (h->after_launch_ev) {
            HIPCHK(h, hipStreamWaitEvent(h->diag_stream, h->after_launch_ev, 0));
        } else {
            HIPCHK(h, hipEventRecord(h->diag_ev, h->stream));
            HIPCHK(h, hipStreamWaitEvent(h->diag_stream, h->diag_ev, 0));
            h->after_launch_ev = h->diag_ev;
        }
        qs = h->diag_stream;
    }
    // Every check works in the handle's one scratch buffer.  Checks on a side stream follow each other there; a check on the
    // compute stream (the call's last slab; demcz_rhat) waits for the latest of them.  (Round 5: a 300-slab demcz_run_checked of
    // four-generation slabs showed the second-to-last check's statistic computed from a scratch the last check was already
    // writing -- one run in four; with 1000-generation slabs the side check is long done when the last slab ends.)
    if (qs == h->stream && h->rhat_side_pending) {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->rhat_side_ev, 0));
        h->rhat_side_pending = false;
    }
    struct SideMark {
        demcz_handle* h; hipStream_t qs;
        ~SideMark() {
            if (qs == h->stream) return;
            if (!h->rhat_side_ev && hipEventCreateWithFlags(&h->rhat_side_ev, hipEventDisableTiming) != hipSuccess) { h->rhat_side_ev = nullptr; return; }
            if (hipEventRecord(h->rhat_side_ev, qs) == hipSuccess) h->rhat_side_pending = true;
        }
    } side_mark{h, qs};
    if (slabs > 1 && h->comm) return fail(h, DEMCZ_ERR_STATE, "demcz_run_checked: batched checks are for unsharded runs");
    int32_t rc = rhat_prepare(h, g_from, g_to, r, true, qs, slabs);
    if (rc) return rc;
    const int d = r.d;
    const int64_t n = r.n;
    const int64_t m = 2 * r.N * h->nranks;                   // utils.jl:5
    const bool sharded = (h->comm != nullptr);
    double* sums = r.sums;               // [0,d): sum_j mean_j; [d,3d): stage-1 sums; [3d,4d): R-hat
    if (!sharded) {
        hipLaunchKernelGGL(rhat_tail_kernel, dim3(d, r.slabs), dim3(256), 0, qs, r.mean_j, r.s2_j, r.N, d, (double)n, (double)m, r.out, r.need);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out, r.out, (size_t)r.slabs * d * sizeof(double), hipMemcpyDeviceToHost, qs));
        return DEMCZ_OK;
    }
    // stage 0 -> all-reduce -> stage 1 with the grand mean formed on the device -> all-reduce ->
    // utils.jl:13-18 on the device: one copy and one synchronisation per check
    const ncclComm_t cq = (qs == h->comm_stream && qs != h->stream) ? h->comm_side : h->comm;
    hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, qs, r.mean_j, r.s2_j, r.N, d, 0, (const double*)nullptr, 1.0, sums);
    HIPCHK(h, hipGetLastError());
    NCCLCHK(h, ncclAllReduce(sums, sums, (size_t)d, ncclDouble, ncclSum, cq, qs));
    hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, qs, r.mean_j, r.s2_j, r.N, d, 1, (const double*)sums, (double)m, sums + d);
    HIPCHK(h, hipGetLastError());
    NCCLCHK(h, ncclAllReduce(sums + d, sums + d, (size_t)2 * d, ncclDouble, ncclSum, cq, qs));
    hipLaunchKernelGGL(rhat_final_kernel, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, qs, (const double*)(sums + d), d, (double)n, (double)m, sums + 3 * d);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, sums + 3 * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, qs));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_rhat(demcz_handle* h, int64_t g_from, int64_t g_to, double* rhat)
{
    if (!h || !rhat) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = live_verify(h);
    if (rc) return rc;
    rc = rhat_enqueue(h, g_from, g_to, rhat);
    if (rc) return rc;
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

// ---- effective sample size (K8, demcz_kernels_acf.h) ------------------------------------------------
// The split chains, their means and the between-chain sum are R-hat's (rhat_prepare, rhat_reduce_kernel); what is new is the
// lagged self-product of every split chain, summed over the chains per (parameter, lag), and Geyer's initial monotone
// sequence over those sums on the host (demcz_ess_from_sums).  Everything runs on the compute stream, on request only.
struct AcfPlan { RhatPlan r; int nchunk, tiles; int64_t per; double *part, *out; };

// Time chunks of one half and lag tiles per launch: a function of (N, d, n) alone, so that a lag's bits do not depend on the
// batch that computes it.  Chunks are whole numbers of tiles long (a trip of the kernel's loop is ACF_TL left samples), at
// least two, and only as many as it takes for 2 halves x 4 tiles x chunks x waves to give every SIMD a few waves.
static void acf_chunks(int64_t N, int d, int64_t n, int& nchunk, int64_t& per)
{
    const int64_t waves = (N * d + ACF_BS - 1) / ACF_BS;
    const int64_t want = (4096 + 8 * waves - 1) / (8 * waves);
    const int64_t k = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n / (2 * ACF_TL), want), 64));
    per = ((n + k - 1) / k + ACF_TL - 1) / ACF_TL * ACF_TL;
    nchunk = (int)((n + per - 1) / per);
}

// live_verify, R-hat's plan for the window, the scratch for it with the chunk partials and one batch of sums behind it, the
// wait for side-stream checks (they work in the same scratch, see rhat_enqueue); launches nothing.
// A launch holds up to four lag tiles, fewer where four tiles of partials would pass 2^24 doubles (128 MB) -- but always one,
// which at one chunk is 64 N d doubles: the size of 64 generations of the history itself.
static int32_t acf_prepare(demcz_handle* h, int64_t g_from, int64_t g_to, AcfPlan& a, const char* who)
{
    int32_t rc = live_verify(h);
    if (rc) return rc;
    rc = rhat_plan(h, g_from, g_to, a.r, who);
    if (rc) return rc;
    RhatPlan& r = a.r;
    acf_chunks(r.N, r.d, r.n, a.nchunk, a.per);
    const int64_t tile = (int64_t)2 * a.nchunk * ACF_TL * r.nd;               // doubles of partials per lag tile
    a.tiles = (int)std::max<int64_t>(1, std::min<int64_t>(4, ((int64_t)1 << 24) / tile));
    rc = rhat_scratch(h, r, a.tiles * tile + (int64_t)a.tiles * ACF_TL * r.d, false);
    if (rc) return rc;
    if (h->rhat_side_pending) {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->rhat_side_ev, 0));
        h->rhat_side_pending = false;
    }
    a.part = h->d_scratch + r.need;
    a.out = a.part + a.tiles * tile;
    return DEMCZ_OK;
}

// Enqueues lags lag_from..lag_to (inside 0..n-1) in launches of a.tiles tiles and the copies of their sums to
// sums[p + d (t - lag_from)]; does not wait.
static int32_t acf_enqueue(demcz_handle* h, const AcfPlan& a, int64_t lag_from, int64_t lag_to, double* sums)
{
    const RhatPlan& r = a.r;
    const unsigned gx = (unsigned)((r.nd + ACF_BS - 1) / ACF_BS);
    for (int64_t t = lag_from; t <= lag_to; t += (int64_t)a.tiles * ACF_TL) {
        const int64_t nl = std::min<int64_t>((int64_t)a.tiles * ACF_TL, lag_to - t + 1);
        const unsigned nz = (unsigned)((nl + ACF_TL - 1) / ACF_TL);
        hipLaunchKernelGGL(acf_products_kernel, dim3(gx, 2 * a.nchunk, nz), dim3(ACF_BS), 0, h->stream, (const double*)h->dchain,
                           (const double*)r.mean_j, r.N, r.d, r.s0, r.n, a.nchunk, a.per, t, a.part);
        hipLaunchKernelGGL(acf_reduce_kernel, dim3(r.d, (unsigned)nl), dim3(256), 0, h->stream, (const double*)a.part, r.N, r.d, a.nchunk,
                           a.out, (int64_t)0);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(sums + (size_t)r.d * (t - lag_from), a.out, (size_t)r.d * nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    return DEMCZ_OK;
}

extern "C" int32_t demcz_autocov_sums(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t lag_from, int64_t lag_to, double* sums)
{
    if (!h || !sums) return DEMCZ_ERR_INVALID_ARGUMENT;
    AcfPlan a;
    int32_t rc = acf_prepare(h, g_from, g_to, a, "demcz_autocov_sums");
    if (rc) return rc;
    if (lag_from < 0 || lag_to < lag_from || lag_to > a.r.n - 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_autocov_sums: 0 <= lag_from <= lag_to <= n - 1, n = half the window");
    rc = rhat_scratch(h, a.r, 0, true);                      // (the scratch is there: this is the split chains' means)
    if (rc) return rc;
    rc = acf_enqueue(h, a, lag_from, lag_to, sums);
    if (rc) return rc;
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_ess_from_sums(int32_t d, int64_t m, int64_t n, int64_t nlags, const double* sums, const double* between,
                                       double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged)
{
    if (d <= 0 || m < 1 || n < 2 || nlags < 1 || !sums || !between || !ess) return DEMCZ_ERR_INVALID_ARGUMENT;
    const double dn = (double)n, dm = (double)m, S = dm * dn;
    const double cap = S * std::log10(S), floor_tau = 1.0 / std::log10(S);
    const int64_t L = nlags - 1;
    for (int p = 0; p < d; ++p) {
        const double A0 = sums[p] / S;
        const double W = A0 * dn / (dn - 1.0);
        const double vp = A0 + between[p] / (dm - 1.0);
        double sum = 0.0, prev = 0.0;
        int64_t k = 0;
        int32_t conv = 0;
        for (; 2 * k + 1 <= L; ++k) {
            const double r0 = k ? 1.0 - (W - sums[p + (size_t)d * (2 * k)] / S) / vp : 1.0;
            const double r1 = 1.0 - (W - sums[p + (size_t)d * (2 * k + 1)] / S) / vp;
            double P = r0 + r1;
            if (!(P > 0.0)) {                       // the stopping pair is not summed; a NaN pair stops too, and shows in tau
                conv = 1;
                if (P != P) sum = P;
                break;
            }
            if (k && prev < P) P = prev;            // initial monotone sequence
            sum += P;
            prev = P;
        }
        const double t = -1.0 + 2.0 * sum;
        ess[p] = (t < floor_tau) ? cap : S / t;
        if (tau) tau[p] = t;
        if (varplus) varplus[p] = vp;
        if (pairs) pairs[p] = k;
        if (converged) converged[p] = conv;
    }
    return DEMCZ_OK;
}

extern "C" int32_t demcz_ess(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t max_lag,
                             double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged)
{
    if (!h || !ess) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->comm && h->nranks > 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_ess: on a sharded handle add demcz_autocov_sums and demcz_rhat_partial over the ranks "
                                                   "on the host and finish with demcz_ess_from_sums");
    AcfPlan a;
    int32_t rc = acf_prepare(h, g_from, g_to, a, "demcz_ess");
    if (rc) return rc;
    rc = rhat_scratch(h, a.r, 0, true);                      // (the scratch is there: this is the split chains' means)
    if (rc) return rc;
    const RhatPlan& r = a.r;
    const int d = r.d;
    const int64_t n = r.n, m = 2 * r.N;
    const int64_t L = (max_lag <= 0) ? n - 1 : std::min<int64_t>(n - 1, max_lag);
    // between[p] = sum_j (mean_j - grand)^2, the grand mean formed on the device as the sharded R-hat forms it
    hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, h->stream, r.mean_j, r.s2_j, r.N, d, 0, (const double*)nullptr, 1.0, r.sums);
    hipLaunchKernelGGL(rhat_reduce_kernel, dim3(d), dim3(256), 0, h->stream, r.mean_j, r.s2_j, r.N, d, 1, (const double*)r.sums, (double)m, r.sums + d);
    HIPCHK(h, hipGetLastError());
    std::vector<double> between((size_t)d), sums;
    std::vector<int32_t> conv((size_t)d);
    HIPCHK(h, hipMemcpyAsync(between.data(), r.sums + d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    // lags in batches of one launch, the finisher after each: it never looks past its stopping pair, so the first batch after
    // which every parameter has stopped gives what all L lags would
    const int64_t batch = (int64_t)a.tiles * ACF_TL;
    int64_t have = 0;
    for (;;) {
        const int64_t to = std::min<int64_t>(L, have + batch - 1);
        sums.resize((size_t)d * (to + 1));
        rc = acf_enqueue(h, a, have, to, sums.data() + (size_t)d * have);
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }       // (copies into this call's vectors may be under way)
        SYNCCHK(h, h->stream);
        have = to + 1;
        rc = demcz_ess_from_sums(d, m, n, have, sums.data(), between.data(), ess, tau, varplus, pairs, conv.data());
        if (rc) return fail(h, rc, "demcz_ess: finisher");
        if (have > L || std::all_of(conv.begin(), conv.end(), [](int32_t c) { return c == 1; })) break;
    }
    if (converged) std::copy(conv.begin(), conv.end(), converged);
    return DEMCZ_OK;
}

// ---- selection (K9, demcz_kernels_sel.h): quantiles by radix select, the best draw ----------------------------------------------
// A counting pass reads the window once and returns integer histograms of one key byte; the host walks the ranks one byte down
// (demcz_select_host.h) and asks for the next byte.  Everything runs on the compute stream, on request only, in scratch that lies
// behind R-hat's plan for the same window, as the autocovariance partials do.
struct SelPlan { int64_t N, w, s0, nd, off, cb, per; int d, nchunk; };

// live_verify, the window, the chunk plan and `extra` doubles of scratch at h->d_scratch + s.off; the wait for side-stream checks.
// Chunks: enough workgroups to fill the chip whatever the shape of the window (as demcz_accept_ratio), at least 16 generations
// each, and never so long that a workgroup's 32-bit bins could wrap (64 chains x 2^20 generations).
static int32_t sel_prepare(demcz_handle* h, int64_t g_from, int64_t g_to, SelPlan& s, int64_t extra, const char* who)
{
    DEADCHK(h);
    int32_t rc = live_verify(h);
    if (rc) return rc;
    rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    s.N = h->cfg.N; s.d = h->cfg.d; s.w = g_to - g_from + 1; s.s0 = g_from - h->g0 - 1; s.nd = s.N * s.d;
    s.off = rhat_need(s.nd, s.d, rhat_chunks(s.w / 2));
    s.cb = (s.N + 63) / 64;
    if (s.cb * s.d > 0x7fffffffll) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": N d too large for one launch");
    const int64_t fill = (4096 + s.cb * s.d - 1) / (s.cb * s.d);
    int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>((s.w + 15) / 16, fill));
    nchunk = std::max<int64_t>(nchunk, (s.w + ((int64_t)1 << 20) - 1) >> 20);
    s.per = (s.w + nchunk - 1) / nchunk;
    s.nchunk = (int)((s.w + s.per - 1) / s.per);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = ensure_scratch(h, s.off + extra);
    if (rc) return rc;
    if (h->rhat_side_pending) {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->rhat_side_ev, 0));
        h->rhat_side_pending = false;
    }
    return DEMCZ_OK;
}

static int sel_width(int nprefix) { int np = 1; while (np < nprefix) np *= 2; return np; }
// doubles of scratch one pass needs: the padded prefixes, the counts and the NaN counts (all 8-byte words)
static int64_t sel_words(int d, int np) { return (int64_t)d * np + (int64_t)d * np * 256 + d; }

template <int NP>
static void sel_launch(demcz_handle* h, const SelPlan& s, int shift, const uint64_t* dpre, unsigned long long* dcnt, unsigned long long* dnan)
{
    hipLaunchKernelGGL(select_counts_kernel<NP>, dim3((unsigned)(s.cb * s.d), (unsigned)s.nchunk), dim3(SEL_BS), 0, h->stream,
                       (const double*)h->dchain, s.N, s.d, s.s0, s.w, s.cb, s.per, shift, dpre, dcnt, dnan);
}

// One pass: uploads the prefixes (hpre: [d][np], padded with ~0; it must live until the stream is synchronised), counts, and
// copies [d][np][256] counts and d NaN counts to hcnt / hnan.  Does not wait.
static int32_t sel_enqueue(demcz_handle* h, const SelPlan& s, int shift, int np, const uint64_t* hpre, uint64_t* hcnt, uint64_t* hnan)
{
    static_assert(sizeof(unsigned long long) == sizeof(double) && sizeof(uint64_t) == sizeof(double), "scratch reuse");
    uint64_t* dpre = reinterpret_cast<uint64_t*>(h->d_scratch + s.off);
    unsigned long long* dcnt = reinterpret_cast<unsigned long long*>(dpre + (size_t)s.d * np);
    unsigned long long* dnan = dcnt + (size_t)s.d * np * 256;
    HIPCHK(h, hipMemcpyAsync(dpre, hpre, (size_t)s.d * np * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(dcnt, 0, ((size_t)s.d * np * 256 + s.d) * sizeof(unsigned long long), h->stream));
    switch (np) {
    case 1: sel_launch<1>(h, s, shift, dpre, dcnt, dnan); break;
    case 2: sel_launch<2>(h, s, shift, dpre, dcnt, dnan); break;
    case 4: sel_launch<4>(h, s, shift, dpre, dcnt, dnan); break;
    case 8: sel_launch<8>(h, s, shift, dpre, dcnt, dnan); break;
    case 16: sel_launch<16>(h, s, shift, dpre, dcnt, dnan); break;
    case 32: sel_launch<32>(h, s, shift, dpre, dcnt, dnan); break;
    default: return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "select_counts: prefix count");
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hcnt, dcnt, (size_t)s.d * np * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hnan, dnan, (size_t)s.d * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_select_counts(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t shift, int32_t nprefix,
                                       const uint64_t* prefix, int64_t* counts, int64_t* nan_count)
{
    if (!h || !prefix || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (nprefix < 1 || nprefix > SEL_MAX_PREFIX || shift < 0 || shift > 56 || shift % 8 != 0)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_select_counts: 1 <= nprefix <= 32, shift a multiple of 8 in 0..56");
    const int np = (shift == 56) ? 1 : sel_width(nprefix);       // at shift 56 every draw matches every prefix: counted once
    SelPlan s;
    int32_t rc = sel_prepare(h, g_from, g_to, s, sel_words(h->cfg.d, np), "demcz_select_counts");
    if (rc) return rc;
    const int d = s.d;
    std::vector<uint64_t> hpre((size_t)d * np, ~(uint64_t)0), hcnt((size_t)d * np * 256), hnan((size_t)d);
    for (int p = 0; p < d; ++p)
        for (int u = 0; u < (shift == 56 ? 1 : nprefix); ++u) hpre[(size_t)p * np + u] = (shift == 56) ? 0 : prefix[p + (size_t)d * u];
    rc = sel_enqueue(h, s, shift, np, hpre.data(), hcnt.data(), hnan.data());
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }          // (copies into this call's vectors may be under way)
    SYNCCHK(h, h->stream);
    for (int p = 0; p < d; ++p)
        for (int u = 0; u < nprefix; ++u)
            for (int b = 0; b < 256; ++b)
                counts[b + 256 * ((size_t)u + (size_t)nprefix * p)] = (int64_t)hcnt[b + 256 * ((size_t)(shift == 56 ? 0 : u) + (size_t)np * p)];
    if (nan_count) for (int p = 0; p < d; ++p) nan_count[p] = (int64_t)hnan[p];
    return DEMCZ_OK;
}

extern "C" int32_t demcz_quantiles(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nq, const double* probs,
                                   double* q, double* lower, double* upper)
{
    if (!h || !probs || !q) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->comm && h->nranks > 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_quantiles: on a sharded handle add demcz_select_counts over the ranks on the host "
                                                   "and step with demcz_select_step");
    if (nq < 1 || nq > SEL_MAX_PROBS) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_quantiles: 1 <= nq <= 16");
    const int nr = 2 * nq;
    SelPlan s;
    int32_t rc = sel_prepare(h, g_from, g_to, s, sel_words(h->cfg.d, sel_width(nr)), "demcz_quantiles");
    if (rc) return rc;
    const int d = s.d;
    std::vector<int64_t> rlo((size_t)nq), rhi((size_t)nq);
    std::vector<double> frac((size_t)nq);
    rc = demcz_quantile_plan(s.N * s.w, nq, probs, rlo.data(), rhi.data(), frac.data());
    if (rc) return fail(h, rc, "demcz_quantiles: every probability must lie in [0, 1]");
    // rank r = 2 j (lower) and 2 j + 1 (upper) of probability j; prefix / rank: [p + d r]
    std::vector<uint64_t> prefix((size_t)d * nr, 0), hpre, hcnt, hnan((size_t)d);
    std::vector<int64_t> rank((size_t)d * nr), cnt((size_t)256 * nr * d), nan((size_t)d);
    std::vector<int> slot((size_t)d * nr);
    for (int p = 0; p < d; ++p)
        for (int j = 0; j < nq; ++j) { rank[p + (size_t)d * (2 * j)] = rlo[j]; rank[p + (size_t)d * (2 * j + 1)] = rhi[j]; }
    for (int shift = 56; shift >= 0; shift -= 8) {
        // the distinct prefixes of each parameter, in order of first appearance; slot[p + d r] = where rank r's prefix went
        int most = 1;
        for (int p = 0; p < d; ++p) {
            int n = 0;
            for (int r = 0; r < nr; ++r) {
                int u = 0;
                while (u < r && prefix[p + (size_t)d * u] != prefix[p + (size_t)d * r]) ++u;
                slot[p + (size_t)d * r] = (u < r) ? slot[p + (size_t)d * u] : n++;
            }
            most = std::max(most, n);
        }
        const int np = (shift == 56) ? 1 : sel_width(most);
        hpre.assign((size_t)d * np, ~(uint64_t)0);
        for (int p = 0; p < d; ++p)
            for (int r = 0; r < nr; ++r) hpre[(size_t)p * np + slot[p + (size_t)d * r]] = prefix[p + (size_t)d * r];
        hcnt.resize((size_t)d * np * 256);
        rc = sel_enqueue(h, s, shift, np, hpre.data(), hcnt.data(), hnan.data());
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
        SYNCCHK(h, h->stream);
        for (int p = 0; p < d; ++p)
            for (int r = 0; r < nr; ++r)
                for (int b = 0; b < 256; ++b)
                    cnt[b + 256 * ((size_t)r + (size_t)nr * p)] = (int64_t)hcnt[b + 256 * ((size_t)slot[p + (size_t)d * r] + (size_t)np * p)];
        rc = demcz_select_step(d, nr, cnt.data(), prefix.data(), rank.data());
        if (rc) return fail(h, rc, "demcz_quantiles: a rank fell outside the counts");
    }
    for (int p = 0; p < d; ++p) nan[p] = (int64_t)hnan[p];
    std::vector<uint64_t> klo((size_t)d * nq), khi((size_t)d * nq);
    for (int p = 0; p < d; ++p)
        for (int j = 0; j < nq; ++j) { klo[p + (size_t)d * j] = prefix[p + (size_t)d * (2 * j)]; khi[p + (size_t)d * j] = prefix[p + (size_t)d * (2 * j + 1)]; }
    return demcz_quantile_finish(d, nq, klo.data(), khi.data(), frac.data(), nan.data(), q, lower, upper);
}

// ---- the best draw: arg-max of log_obj over the window -----------------------------------------------------------------------
extern "C" int32_t demcz_best(demcz_handle* h, int64_t g_from, int64_t g_to, double* bestval, int64_t* chain, int64_t* generation,
                              double* bestpar)
{
    NOT_DERIVED(h);
    if (!h || !bestval || !chain || !generation) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_best");
    if (rc) return rc;
    const int64_t total = h->cfg.N * (g_to - g_from + 1);
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((total + 2047) / 2048, 1024));
    SelPlan s;                       // (of the plan only the window and the scratch offset are used here)
    rc = sel_prepare(h, g_from, g_to, s, 2 * (int64_t)nb + 2, "demcz_best");
    if (rc) return rc;
    if (bestpar && !h->dchain) return fail(h, DEMCZ_ERR_STATE, "demcz_best: no chain history to take bestpar from");
    static_assert(sizeof(long long) == sizeof(double), "scratch reuse");
    double* pv = h->d_scratch + s.off;
    long long* pi = reinterpret_cast<long long*>(pv + nb);
    double* ov = pv + 2 * (size_t)nb;
    long long* oi = reinterpret_cast<long long*>(ov + 1);
    hipLaunchKernelGGL(best_partial_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, (const double*)(h->dlogobj + (size_t)s.N * s.s0), total, pv, pi);
    hipLaunchKernelGGL(best_final_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)pv, (const long long*)pi, nb, ov, oi);
    HIPCHK(h, hipGetLastError());
    double v = 0.0;
    long long i = -1;
    HIPCHK(h, hipMemcpyAsync(&v, ov, sizeof v, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&i, oi, sizeof i, hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(h, h->stream);
    *bestval = v;
    if (i < 0) {
        *chain = -1; *generation = -1;
        if (bestpar) for (int p = 0; p < s.d; ++p) bestpar[p] = std::nan("");
        return DEMCZ_OK;
    }
    *chain = i % s.N;
    *generation = g_from + i / s.N;
    if (bestpar) {
        HIPCHK(h, hipMemcpy2DAsync(bestpar, sizeof(double), h->dchain + (size_t)(i % s.N) + (size_t)s.nd * (s.s0 + i / s.N),
                                   (size_t)s.N * sizeof(double), sizeof(double), (size_t)s.d, hipMemcpyDeviceToHost, h->stream));
        SYNCCHK(h, h->stream);
    }
    return DEMCZ_OK;
}

extern "C" int32_t demcz_accept_ratio(demcz_handle* h, int64_t g_from, int64_t g_to, double* ratio)
{
    NOT_DERIVED(h);
    if (!h || !ratio) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_accept_ratio");
    if (rc) return rc;
    const int64_t N = h->cfg.N, w = g_to - g_from + 1, s0 = g_from - h->g0 - 1;
    if (w < 2) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_accept_ratio: need at least 2 generations");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = live_verify(h);
    if (rc) return rc;
    rc = ensure_scratch(h, 2 * N);
    if (rc) return rc;
    {   // chains x time chunks: enough workgroups to fill the chip whatever the shape of the window
        const int64_t cb = (N + 63) / 64;
        const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((w - 1 + 31) / 32, 1024), (4096 + cb - 1) / cb));
        unsigned int* cnt = reinterpret_cast<unsigned int*>(h->d_scratch + N);
        HIPCHK(h, hipMemsetAsync(cnt, 0, (size_t)N * sizeof(unsigned int), h->stream));
        hipLaunchKernelGGL(changed_per_chain_kernel, dim3((unsigned)cb, (unsigned)nchunk), dim3(64), 0, h->stream, h->dlogobj, N, s0, w, nchunk, cnt);
        hipLaunchKernelGGL(changed_ratio_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (const unsigned int*)cnt, N, w, h->d_scratch);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(ratio, h->d_scratch, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(h, h->stream);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_mean_cov(demcz_handle* h, int64_t g_from, int64_t g_to, double* mean, double* cov)
{
    if (!h || !mean || !cov) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = check_hist_range(h, g_from, g_to, "demcz_mean_cov");
    if (rc) return rc;
    const int64_t N = h->cfg.N, w = g_to - g_from + 1, s0 = g_from - h->g0 - 1;
    const int d = h->cfg.d;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = live_verify(h);
    if (rc) return rc;
    const int T = (d + MC_TS - 1) / MC_TS, npair = T * (T + 1) / 2;
    const int64_t cb = (N + 255) / 256;
    const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((w + 15) / 16, 512), (2048 + cb * npair - 1) / (cb * npair)));
    const int64_t nblk_xy = cb * nchunk;
    rc = ensure_scratch(h, (int64_t)d * (d + 1) + d + nblk_xy * npair * MC_VALS);
    if (rc) return rc;
    double* sums = h->d_scratch;
    double* partial = sums + (int64_t)d * (d + 1) + d;
    hipLaunchKernelGGL(meancov_partial_kernel, dim3((unsigned)cb, (unsigned)nchunk, (unsigned)npair), dim3(256), 0, h->stream,
                       (const double*)h->dchain, N, d, s0, w, nchunk, partial);
    hipLaunchKernelGGL(meancov_final_kernel, dim3((unsigned)((d * (d + 1) + 63) / 64)), dim3(64), 0, h->stream, (const double*)partial, d,
                       (int)nblk_xy, sums);
    HIPCHK(h, hipGetLastError());
    std::vector<double> hs((size_t)d * (d + 1)), ref((size_t)d);
    HIPCHK(h, hipMemcpyAsync(hs.data(), sums, hs.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(ref.data(), sizeof(double), h->dchain + (size_t)N * d * s0, (size_t)N * sizeof(double),
                               sizeof(double), (size_t)d, hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(h, h->stream);
    const double cnt = (double)(N * w);
    std::vector<double> dm((size_t)d);      // mean - ref
    for (int p = 0; p < d; ++p) { dm[p] = hs[(size_t)p + (size_t)d * d] / cnt; mean[p] = ref[p] + dm[p]; }
    for (int p = 0; p < d; ++p)
        for (int q = 0; q < d; ++q) cov[p + d * q] = hs[(size_t)p + (size_t)d * q] / cnt - dm[p] * dm[q];   // utils.jl:104
    return DEMCZ_OK;
}

// ---- host-closure mode -------------------------------------------------------------------------
namespace demcz {
// (host_X / done_count / host_flag: the pipelined closure mode, demcz_closure_buffers -- the proposals also go to pinned host memory,
//  and the last workgroup to finish publishes `seq` in the flag word the host is spinning on)
__device__ __forceinline__ void propose_done(unsigned int* done_count, unsigned int* host_flag, unsigned int seq)
{
    if (!host_flag) return;
    __threadfence_system();                       // this thread's stores to host memory, before the workgroup reports
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int prev = __hip_atomic_fetch_add(done_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(done_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (ready for the next launch)
            __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
__global__ void propose_kernel(const WindowParams P, int ib, uint64_t blk0, double* Xprop, double* logu, double* host_X,
                               unsigned int* done_count, unsigned int* host_flag, unsigned int seq)
{
    extern __shared__ double lds[];
    const int64_t c = (int64_t)blockIdx.x * WINDOW_BS + threadIdx.x;
    if (c >= P.N) { propose_done(done_count, host_flag, seq); return; }
    const int tid = threadIdx.x;
    const int d = P.d;
    rng_state st;
    rng_seek(st, P.seed, (uint64_t)(P.chain_id0 + c), blk0);
    uint64_t r1, r2, i1, i2;
    rng_next(st, r1, r2);
    draw_rows(r1, r2, (uint64_t)P.M, i1, i2);
    const int b = P.block_offsets[ib + 1] - P.block_offsets[ib];
    const int nn = (b == 1) ? 1 : b;
    const int npairs = (nn + 1) / 2;
    for (int pr = 0; pr < npairs; ++pr) {
        rng_next(st, r1, r2);
        double z0, z1;
        normal_pair(r1, r2, z0, z1);
        lds[(2 * pr) * WINDOW_BS + tid] = z0;
        lds[(2 * pr + 1) * WINDOW_BS + tid] = z1;
    }
    const double scale = (b == 1) ? P.gamma : P.gamma / sqrt((double)(2 * b));
    const int32_t* so = P.slot_of + ib * d;
    const double* za = P.Z + (int64_t)i1 * P.ZS;
    const double* zb = P.Z + (int64_t)i2 * P.ZS;
    for (int p = 0; p < d; ++p) {
        const int t = so[p];
        double xv = P.Xcur[c + P.N * p];
        if (t >= 0) {
            double diff = za[p] - zb[p];
            double zt = lds[((b == 1) ? 0 : t) * WINDOW_BS + tid];
            double t1 = scale * diff;
            double t2 = P.eps[p] * zt;
            double delta = t1 + t2;
            xv = xv + delta;
        }
        Xprop[c + P.N * p] = xv;
        if (host_X) host_X[c + P.N * p] = xv;
    }
    rng_next(st, r1, r2);
    logu[c] = dm_log(u_open(r1));
    propose_done(done_count, host_flag, seq);
}

__global__ void accept_commit_kernel(int64_t N, int d, double* Xcur, double* lpcur, const double* Xprop,
                                     const double* lpprop, const double* logu, int has_T, double T)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double lp = lpcur[c], lpp = lpprop[c];
    double dlt = lpp - lp;
    if (has_T) dlt = dlt / T;
    if (logu[c] < dlt) {
        for (int p = 0; p < d; ++p) Xcur[c + N * p] = Xprop[c + N * p];
        lpcur[c] = lpp;
    }
}

__global__ void end_generation_kernel(int64_t N, int d, const double* Xcur, const double* lpcur,
                                      double* chain, double* logobj, int64_t slot,
                                      double* Z, int64_t ZS, int64_t M, int do_append)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    for (int p = 0; p < d; ++p) {
        const double xv = Xcur[c + N * p];
        if (chain) chain[c + N * (p + (int64_t)d * slot)] = xv;
        if (do_append) Z[(M + c) * ZS + p] = xv;
    }
    if (logobj) logobj[c + N * slot] = lpcur[c];
}
}  // namespace demcz

extern "C" int32_t demcz_propose(demcz_handle* h, int64_t g, int32_t ib, double gamma, double* Xprop)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->cr_ncr > 0) return fail(h, DEMCZ_ERR_STATE, "demcz_propose: the handle has crossover generations (demcz_set_crossover): the closure mode has no crossover");
    if (h->cfg.target_kind != DEMCZ_TARGET_HOST_CALLBACK) return fail(h, DEMCZ_ERR_STATE, "demcz_propose: handle was not created with DEMCZ_TARGET_HOST_CALLBACK");
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_propose: call demcz_set_state first");
    if (g < 1 || ib < 0 || ib >= h->cfg.Nblocks) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_propose: bad generation or block");
    if (h->proposal_pending) return fail(h, DEMCZ_ERR_STATE, "demcz_propose: previous proposal not committed");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int64_t N = h->cfg.N;
    const int d = h->cfg.d;
    int64_t off = 0;
    for (int t = 0; t < ib; ++t) off += blockstep_nblk(h->block_offsets[t + 1] - h->block_offsets[t]);
    WindowParams P{};
    P.Z = h->dZ; P.ZS = h->ZS; P.M = h->M; P.Xcur = h->dX; P.N = N; P.chain_id0 = h->cfg.chain_id0; P.d = d;
    P.gamma = gamma; P.seed = h->cfg.seed; P.block_offsets = h->d_block_offsets; P.slot_of = h->d_slot_of; P.eps = h->d_eps;
    const uint64_t blk0 = (uint64_t)(g + h->rng_offset - 1) * (uint64_t)h->S + (uint64_t)off;
    if (h->hc_X) {
        // pipelined: the kernel writes the proposals into pinned host memory itself and raises the flag; the host spins on it
        const unsigned int seq = ++h->hc_seq;
        double* hX = nullptr; unsigned int* hF = nullptr;
        HIPCHK(h, hipHostGetDevicePointer((void**)&hX, h->hc_X, 0));
        HIPCHK(h, hipHostGetDevicePointer((void**)&hF, const_cast<unsigned int*>(h->hc_flag), 0));
        hipLaunchKernelGGL(propose_kernel, dim3((unsigned)((N + WINDOW_BS - 1) / WINDOW_BS)), dim3(WINDOW_BS),
                           (size_t)(d + 1) * WINDOW_BS * sizeof(double), h->stream, P, (int)ib, blk0, h->dXprop, h->dlogu, hX, h->hc_count, hF, seq);
        HIPCHK(h, hipGetLastError());
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned long long polls = 0; __atomic_load_n(const_cast<unsigned int*>(h->hc_flag), __ATOMIC_ACQUIRE) != seq; ++polls) {
            if ((polls & 0xffffull) == 0xffffull) {       // (now and then: did the launch fail?  is a sharded peer stalling the stream?)
                const hipError_t qe = hipStreamQuery(h->stream);
                if (qe != hipSuccess && qe != hipErrorNotReady) return fail(h, DEMCZ_ERR_HIP, std::string("demcz_propose: ") + hipGetErrorString(qe));
                if (qe == hipSuccess && __atomic_load_n(const_cast<unsigned int*>(h->hc_flag), __ATOMIC_ACQUIRE) != seq)
                    return fail(h, DEMCZ_ERR_HIP, "demcz_propose: the propose kernel finished without raising its flag");
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) return fail(h, DEMCZ_ERR_HIP, "demcz_propose: no proposal within 60 s");
            }
        }
        if (Xprop && Xprop != h->hc_X) std::memcpy(Xprop, h->hc_X, (size_t)N * d * sizeof(double));
    } else {
        if (!Xprop) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_propose: Xprop is required (or call demcz_closure_buffers first)");
        hipLaunchKernelGGL(propose_kernel, dim3((unsigned)((N + WINDOW_BS - 1) / WINDOW_BS)), dim3(WINDOW_BS),
                           (size_t)(d + 1) * WINDOW_BS * sizeof(double), h->stream, P, (int)ib, blk0, h->dXprop, h->dlogu,
                           (double*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, 0u);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(Xprop, h->dXprop, (size_t)N * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        SYNCCHK(h, h->stream);
    }
    h->gen_open = true;                           // (only a proposal that was made opens a generation: a refused call leaves none)
    h->proposal_pending = true;
    return DEMCZ_OK;
}

// Pinned host buffers for the closure mode: *Xprop (N x d column-major, ld N) receives every proposal of demcz_propose, *logp (N) is
// where the caller leaves the closure's values for demcz_accept_commit -- the kernels read and write them in place (see
// demcz_handle::hc_X).  The buffers belong to the handle and live as long as it does.
extern "C" int32_t demcz_closure_buffers(demcz_handle* h, double** Xprop, double** logp)
{
    NOT_DERIVED(h);
    if (!h || !Xprop || !logp) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->cfg.target_kind != DEMCZ_TARGET_HOST_CALLBACK) return fail(h, DEMCZ_ERR_STATE, "demcz_closure_buffers: handle was not created with DEMCZ_TARGET_HOST_CALLBACK");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->hc_X) {
        const size_t N = (size_t)h->cfg.N, d = (size_t)h->cfg.d;
        double* x = nullptr; double* l = nullptr; unsigned int* f = nullptr;
        if (hipHostMalloc((void**)&x, N * d * sizeof(double), hipHostMallocMapped) != hipSuccess ||
            hipHostMalloc((void**)&l, N * sizeof(double), hipHostMallocMapped) != hipSuccess ||
            hipHostMalloc((void**)&f, 64, hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            if (x) (void)hipHostFree(x);
            if (l) (void)hipHostFree(l);
            if (f) (void)hipHostFree(f);
            return fail(h, DEMCZ_ERR_HIP, "demcz_closure_buffers: pinned allocation failed");
        }
        std::memset(x, 0, N * d * sizeof(double)); std::memset(l, 0, N * sizeof(double)); std::memset(f, 0, 64);
        HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->hc_count, sizeof(unsigned int)));
        HIPCHK(h, hipMemsetAsync(h->hc_count, 0, sizeof(unsigned int), h->stream));
        h->hc_X = x; h->hc_lp = l; h->hc_flag = f;
    }
    *Xprop = h->hc_X;
    *logp = h->hc_lp;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_accept_commit(demcz_handle* h, const double* logp_prop, const double* temperature)
{
    NOT_DERIVED(h);
    if (!h || (!logp_prop && !h->hc_lp)) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->proposal_pending) return fail(h, DEMCZ_ERR_STATE, "demcz_accept_commit: no pending proposal");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int64_t N = h->cfg.N;
    if (h->hc_lp) {
        // pipelined: the kernel reads the log-densities from pinned host memory; nothing is waited for -- the next demcz_propose is
        // enqueued behind this kernel, and the caller does not write the buffer again before that proposal has come back
        if (logp_prop && logp_prop != h->hc_lp) std::memcpy(h->hc_lp, logp_prop, (size_t)N * sizeof(double));
        double* lpd = nullptr;
        HIPCHK(h, hipHostGetDevicePointer((void**)&lpd, h->hc_lp, 0));
        hipLaunchKernelGGL(accept_commit_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, N, h->cfg.d, h->dX,
                           h->dlp, h->dXprop, (const double*)lpd, h->dlogu, temperature ? 1 : 0, temperature ? *temperature : 1.0);
        HIPCHK(h, hipGetLastError());
        h->proposal_pending = false;
        return DEMCZ_OK;
    }
    int32_t rc = ensure_scratch(h, N);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch, logp_prop, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(accept_commit_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, N, h->cfg.d, h->dX,
                       h->dlp, h->dXprop, h->d_scratch, h->dlogu, temperature ? 1 : 0, temperature ? *temperature : 1.0);
    HIPCHK(h, hipGetLastError());
    SYNCCHK(h, h->stream);
    h->proposal_pending = false;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_end_generation(demcz_handle* h, int64_t g)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->cfg.target_kind != DEMCZ_TARGET_HOST_CALLBACK) return fail(h, DEMCZ_ERR_STATE, "demcz_end_generation: host-callback handles only");
    if (h->proposal_pending || !h->gen_open) return fail(h, DEMCZ_ERR_STATE, "demcz_end_generation: no open generation or uncommitted proposal");
    const bool hist = h->cfg.Gcap > 0;
    if (hist && (g - h->g0 - 1 < 0 || g - h->g0 > h->cfg.Gcap)) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_end_generation: outside the history window");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int64_t N = h->cfg.N;
    const bool boundary = (g % h->cfg.K) == 0;
    const bool sharded = (h->comm != nullptr);
    const bool kappend = boundary && !sharded && !h->external_append;
    if (h->lag != 0) return fail(h, DEMCZ_ERR_STATE, "demcz_end_generation: the host-closure path runs with append lag 0");
    if (kappend && h->M_app + N > h->cfg.Mcap) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_end_generation: Z capacity exceeded");
    hipLaunchKernelGGL(end_generation_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, N, h->cfg.d, h->dX, h->dlp,
                       hist ? h->dchain : nullptr, hist ? h->dlogobj : nullptr,
                       hist ? (g - h->g0 - 1) : 0, h->dZ, h->ZS, h->M, kappend ? 1 : 0);
    HIPCHK(h, hipGetLastError());
    if (kappend) { h->M_app += N; h->M = h->M_app; }
    else if (boundary && sharded) { int32_t rc = append_after_window(h); if (rc) return rc; }
    h->gen_open = false;
    h->g_done = g;
    return DEMCZ_OK;
}

// ---- multi-GPU -------------------------------------------------------------------------------------
extern "C" int32_t demcz_comm_unique_id(void* unique_id_128B)
{
    if (!unique_id_128B) return DEMCZ_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, DEMCZ_ERR_HIP, "ncclGetUniqueId failed");
    std::memcpy(unique_id_128B, &id, sizeof(id));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_comm_init(demcz_handle* h, const void* unique_id_128B, int32_t nranks, int32_t rank)
{
    NOT_DERIVED(h);
    if (!h || !unique_id_128B || nranks < 1 || rank < 0 || rank >= nranks) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->comm) return fail(h, DEMCZ_ERR_STATE, "demcz_comm_init: communicator already initialised");
    if (h->prog_wave)
        return fail(h, DEMCZ_ERR_STATE, "demcz_comm_init: a program target on DEMCZ_LAYOUT_PROGRAM_WAVE does not join a communicator (sharded in-launch "
                                        "hand-off is not built for programs): shard it from the host (demcz_set_external_append, demcz_append_rows) "
                                        "or use the one-lane layout");
    if (!h->live_log.empty()) { int32_t rcv = live_verify(h); if (rcv) return rcv; }
    if (h->cfg.chain_id0 != (int64_t)rank * h->cfg.N)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_comm_init: chain_id0 must be rank * N (equal shards in rank order)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    ncclUniqueId id;
    std::memcpy(&id, unique_id_128B, sizeof(id));
    NCCLCHK(h, ncclCommInitRank(&h->comm, nranks, id, rank));
    h->nranks = nranks;
    h->rank = rank;
    if (const char* tenv = getenv("DEMCZ_COMM_TIMEOUT_MS")) h->comm_timeout_ms = std::max<long long>(0, atoll(tenv));
    HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_gather, (size_t)h->cfg.N * h->cfg.d * nranks * sizeof(double)));
    return peer_setup_ipc(h);
}

// ---- replicas that publish into each other (round 4) ----------------------------------------------------------------------------
extern "C" int32_t demcz_peer_group(demcz_handle** handles, int32_t R)
{
    if (!handles || R < 2 || R > DEMCZ_MAX_PEERS + 1) return DEMCZ_ERR_INVALID_ARGUMENT;
    demcz_handle* h0 = handles[0];
    if (!h0) return DEMCZ_ERR_INVALID_ARGUMENT;
    for (int r = 0; r < R; ++r) {
        demcz_handle* m = handles[r];
        if (!m) return DEMCZ_ERR_INVALID_ARGUMENT;
        NOT_DERIVED(m);
        for (int q = 0; q < r; ++q) if (handles[q] == m) return fail(m, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_peer_group: a handle appears twice");
        if (m->comm || m->peer_mode != 0) return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: handle is already sharded");
        if (m->snooker_every > 0) return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: a handle with snooker generations (demcz_set_snooker) does not join a replica group");
        if (m->cr_ncr > 0) return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: a handle with crossover generations (demcz_set_crossover) does not join a replica group");
        if (m->prog_wave)
            return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: a program target on DEMCZ_LAYOUT_PROGRAM_WAVE does not join a replica group (sharded "
                                            "in-launch hand-off is not built for programs): shard it from the host or use the one-lane layout");
        if (m->lag != 0 || m->external_append) return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: append lag 0 and library-owned appends only");
        if (!m->live_log.empty()) { int32_t rcv = live_verify(m); if (rcv) return rcv; }
        if (m->cfg.device_id != h0->cfg.device_id || m->cfg.N != h0->cfg.N || m->cfg.d != h0->cfg.d || m->cfg.K != h0->cfg.K ||
            m->cfg.Mcap != h0->cfg.Mcap || m->cfg.seed != h0->cfg.seed || m->ZS != h0->ZS || m->lanes != h0->lanes ||
            m->split_kind != h0->split_kind || m->cfg.target_kind != h0->cfg.target_kind || m->cfg.Nblocks != h0->cfg.Nblocks)
            return fail(m, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_peer_group: the members must be shards of ONE run: same device, N, d, K, Mcap, seed, target, layout");
        if (m->cfg.chain_id0 != (int64_t)r * m->cfg.N)
            return fail(m, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_peer_group: chain_id0 of member r must be r * N (equal shards in rank order)");
        if (m->M != h0->M || m->M_app != h0->M_app || m->g_done != h0->g_done)
            return fail(m, DEMCZ_ERR_STATE, "demcz_peer_group: the members' archives / generation counters differ");
    }
    // The members' launches wait for each other's rows, so they must be able to RUN at the same time.  HIP multiplexes its streams
    // over a few hardware queues (GPU_MAX_HW_QUEUES, four by default), and two kernels on one hardware queue run one after the
    // other whatever streams they came from: two members whose streams share a queue would wait for each other until the poll
    // limit.  So: a rendezvous kernel on every member's stream (each waits, at most 2 ms, until all R have started); if they do
    // not all meet, the members that own their stream get fresh ones (a new stream goes to the least used queue) and the
    // rendezvous is tried again.  No luck after a few rounds: the group runs in lockstep from the start (G->failed).
    bool concurrent = false;
    {
        unsigned int* d_rv = nullptr;
        HIPCHK(h0, hipSetDevice(h0->cfg.device_id));
        HIPCHK(h0, dev_malloc(h0->cfg.device_id, (void**)&d_rv, 2 * sizeof(unsigned int)));
        std::vector<hipStream_t> spare;
        for (int round = 0; round < 6 && !concurrent; ++round) {
            if (hipMemset(d_rv, 0, 2 * sizeof(unsigned int)) != hipSuccess) break;
            for (int r = 0; r < R; ++r)
                hipLaunchKernelGGL(rendezvous_kernel, dim3(1), dim3(1), 0, handles[r]->stream, d_rv, (unsigned int)R, d_rv + 1, 200000ull);
            bool okl = hipGetLastError() == hipSuccess;
            for (int r = 0; r < R; ++r) okl = (hipStreamSynchronize(handles[r]->stream) == hipSuccess) && okl;
            unsigned int rv[2] = {0, 0};
            if (!okl || hipMemcpy(rv, d_rv, sizeof(rv), hipMemcpyDeviceToHost) != hipSuccess) break;
            if (rv[1] == (unsigned int)R) { concurrent = true; break; }
            for (int r = 0; r < R; ++r) {
                demcz_handle* m = handles[r];
                if (!m->own_stream) continue;
                hipStream_t ns = nullptr;
                if (hipStreamCreateWithFlags(&ns, hipStreamNonBlocking) != hipSuccess) continue;
                spare.push_back(m->stream);             // (kept alive until the group's streams are settled: the queue
                m->stream = ns;                          //  assignment of the next new stream depends on what exists)
                m->after_launch_ev = nullptr;
            }
        }
        for (hipStream_t st : spare) stream_release(h0->cfg.device_id, st, true);
        (void)dev_free(h0->cfg.device_id, d_rv);
    }
    PeerGroup* G = new PeerGroup();
    for (int r = 0; r < R; ++r) G->members.push_back(handles[r]);
    G->rearms_left = h0->live_rearms_left;
    for (int r = 0; r < R; ++r) {
        demcz_handle* m = handles[r];
        peer_no_dual(m);
        m->group = G;
        m->peer_mode = 1;
        m->nranks = R;
        m->rank = r;
        m->n_peers = 0;
        for (int q = 0; q < R; ++q) if (q != r) m->peer_Z[m->n_peers++] = handles[q]->dZ;
        rec_invalidate(m);                  // (draws made against N rows per boundary no longer apply)
    }
    // Hand-off inside the launches: a layout that has it, streams that can overlap -- and EVERY member able to issue LIVE launches
    // (its shard within what a launch may hold, its share of the device's LIVE budget granted).  All of them or none: a member
    // without LIVE launches only logs its calls (demcz_run), and they are executed for the whole group, in lockstep, at the next
    // verification -- which group_verify does when the group is marked `failed`.
    bool all_live = peer_capable(h0) && concurrent;
    for (int r = 0; r < R && all_live; ++r) all_live = live_span(handles[r]) > 0;
    if (!all_live) for (int r = 0; r < R; ++r) live_release(handles[r]);
    G->lockstep_only = !all_live;
    G->failed = G->lockstep_only;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_peer_status(const demcz_handle* h, int32_t* mode, int32_t* peers)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (mode) *mode = h->peer_mode;
    if (peers) *peers = h->n_peers;
    return DEMCZ_OK;
}

// The archive moves into a fine-grained allocation of its own (coherent for writers on other GPUs while kernels run; the pool's
// buffers are ordinary coarse-grained device memory), with whatever it -- and, in the arena, the record buffers behind it --
// already holds (set_state may have run), and is exported with hipIpcGetMemHandle.  `ok` = false: an allocation flag or IPC
// refused; the handle is unchanged then.
static int32_t archive_make_fine(demcz_handle* h, hipIpcMemHandle_t* mh, bool* ok)
{
    *ok = false;
    if (h->archive_fine) {
        *ok = hipIpcGetMemHandle(mh, h->dZ) == hipSuccess;
        if (!*ok) (void)hipGetLastError();
        return DEMCZ_OK;
    }
    double* fine = nullptr;
    const size_t box_off = (h->dZ_bytes + 255) & ~(size_t)255;
    if (hipExtMallocWithFlags((void**)&fine, box_off + PEER_MAILBOX_BYTES, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); return DEMCZ_OK; }
    if (hipIpcGetMemHandle(mh, fine) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(fine); return DEMCZ_OK; }
    { int32_t rcq = quiesce_all(h); if (rcq) { (void)hipFree(fine); return rcq; } }
    if (h->prod_stream) (void)hipStreamSynchronize(h->prod_stream);
    if (hipMemcpyAsync(fine, h->dZ, h->dZ_bytes, hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
        hipMemsetAsync(reinterpret_cast<unsigned char*>(fine) + box_off, 0, PEER_MAILBOX_BYTES, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipFree(fine);
        return fail(h, DEMCZ_ERR_HIP, "copy into the fine-grained archive failed");
    }
    rec_invalidate(h);
    const ptrdiff_t shift = reinterpret_cast<unsigned char*>(fine) - reinterpret_cast<unsigned char*>(h->dZ);
    auto rebase = [&](double*& q) { if (q) q = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(q) + shift); };
    if (h->arena) {
        rebase(h->arena_rec[0]); rebase(h->arena_rec[1]); rebase(h->arena_temp);
        if (h->rec_in_arena) { rebase(h->d_rec[0]); rebase(h->d_rec[1]); }
    }
    g_dev_pool.release(h->dZ, h->cfg.device_id);
    h->dZ = fine;
    h->archive_fine = true;
    h->mailbox_off = box_off;
    *ok = true;
    return DEMCZ_OK;
}

// opens the other ranks' archives (handles in rank order, this rank's own skipped); all or nothing
static bool peers_open(demcz_handle* h, const hipIpcMemHandle_t* handles, int R, int rank)
{
    void* mapped[DEMCZ_MAX_PEERS] = {nullptr};
    int nmap = 0;
    for (int r = 0; r < R; ++r) {
        if (r == rank) continue;
        void* ptr = nullptr;
        if (hipIpcOpenMemHandle(&ptr, handles[r], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            (void)hipGetLastError();
            for (int i = 0; i < nmap; ++i) (void)hipIpcCloseMemHandle(mapped[i]);
            return false;
        }
        mapped[nmap++] = ptr;
    }
    for (int i = 0; i < nmap; ++i) { h->ipc_mapped[i] = mapped[i]; h->peer_Z[i] = reinterpret_cast<double*>(mapped[i]); }
    h->n_peers = nmap;
    return true;
}

// demcz_comm_init, second half: every rank's archive becomes a fine-grained allocation of its own, its IPC handle travels in one
// ncclAllGather, and every rank opens the other ranks' archives.  Any refusal anywhere (an allocation flag, IPC, peer access)
// switches the mode off on ALL ranks (min-reduced), and the run exchanges its rows through ncclAllGather as before.  Returns
// DEMCZ_OK either way unless the communicator itself fails.
static int32_t peer_setup_ipc(demcz_handle* h)
{
    const bool off = getenv("DEMCZ_NO_PEER") != nullptr;
    const bool self = getenv("DEMCZ_PEER_SELF") != nullptr;      // a one-rank communicator walks the path too (tests)
    const int R = h->nranks;
    if (off || R > DEMCZ_MAX_PEERS + 1 || (R < 2 && !self)) return DEMCZ_OK;
    HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_err_all, 4 * sizeof(unsigned int)));
    HIPCHK(h, hipMemsetAsync(h->d_err_all, 0, 4 * sizeof(unsigned int), h->stream));
    struct Rec { hipIpcMemHandle_t mh; int32_t ok; int32_t pad; };
    static_assert(sizeof(Rec) % 8 == 0, "all-gather record");
    Rec mine{};
    if (peer_capable(h)) {
        bool okf = false;
        int32_t rcf = archive_make_fine(h, &mine.mh, &okf);
        if (rcf) return rcf;
        mine.ok = okf ? 1 : 0;
    }
    Rec* d_rec = nullptr;
    HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&d_rec, sizeof(Rec) * (size_t)(R + 1)));
    std::vector<Rec> all((size_t)R);
    int32_t rc = DEMCZ_OK;
    auto cleanup = [&]() { if (d_rec) (void)dev_free(h->cfg.device_id, d_rec); };
    if (hipMemcpyAsync(d_rec + R, &mine, sizeof(Rec), hipMemcpyHostToDevice, h->stream) != hipSuccess) { cleanup(); return fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: upload failed"); }
    if (ncclAllGather(d_rec + R, d_rec, sizeof(Rec), ncclChar, h->comm, h->stream) != ncclSuccess) { cleanup(); return fail(h, DEMCZ_ERR_COMM, "demcz_comm_init: all-gather of the IPC handles failed"); }
    rc = sync_stream(h, h->stream, "demcz_comm_init (IPC handles)");
    if (rc == DEMCZ_OK && hipMemcpy(all.data(), d_rec, sizeof(Rec) * (size_t)R, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: download failed");
    if (rc) { cleanup(); return rc; }
    unsigned int ok = 1u;
    for (int r = 0; r < R; ++r) ok &= all[(size_t)r].ok ? 1u : 0u;
    if (ok) {
        std::vector<hipIpcMemHandle_t> hs((size_t)R);
        for (int r = 0; r < R; ++r) hs[(size_t)r] = all[(size_t)r].mh;
        ok = peers_open(h, hs.data(), R, h->rank) ? 1u : 0u;
    }
    // every rank must have opened every archive, or nobody uses any
    unsigned int* d_ok = reinterpret_cast<unsigned int*>(d_rec);
    if (hipMemcpyAsync(d_ok, &ok, sizeof(ok), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        ncclAllReduce(d_ok, d_ok, 1, ncclUint32, ncclMin, h->comm, h->stream) != ncclSuccess) rc = fail(h, DEMCZ_ERR_COMM, "demcz_comm_init: reduction failed");
    if (rc == DEMCZ_OK) rc = sync_stream(h, h->stream, "demcz_comm_init (IPC agreement)");
    unsigned int all_ok = 0u;
    if (rc == DEMCZ_OK && hipMemcpy(&all_ok, d_ok, sizeof(all_ok), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: download failed");
    auto close_all = [&]() {
        for (int i = 0; i < DEMCZ_MAX_PEERS; ++i) if (h->ipc_mapped[i]) { (void)hipIpcCloseMemHandle(h->ipc_mapped[i]); h->ipc_mapped[i] = nullptr; }
        h->n_peers = 0;
    };
    if (rc || !all_ok) {
        cleanup();
        close_all();
        return rc;
    }
    // Second agreement (round 5), two questions in one reduction:
    //  * first contact (peer_ping_kernel): does a token stored from every peer's running kernel reach this rank's polling kernel
    //    through the mappings just opened, within 200 ms?  The hand-off has only ever run between processes on ONE GPU before
    //    a multi-GPU node sees it; this asks the links themselves, before any row depends on the answer;
    //  * can THIS rank issue LIVE launches at all -- live_span() depends on the process's LIVE budget on its device (another handle
    //    of the process may hold it) and on the occupancy query?  A rank that exchanged through ncclAllGather
    //    while its peers publish and poll would stall all of them until the communicator's deadline.
    // Either every rank hands its rows over inside the launches, or none does.
    h->peer_mode = 2;
    peer_no_dual(h);
    unsigned int* d_res = reinterpret_cast<unsigned int*>(d_rec) + 4;
    unsigned int agree = 1u;
    {
        PingBoxes pb{};
        for (int i = 0; i < h->n_peers; ++i) pb.box[i] = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(h->peer_Z[i]) + h->mailbox_off);
        unsigned long long* own = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(h->dZ) + h->mailbox_off);
        static const unsigned long long ping_ms = getenv("DEMCZ_PING_MS") ? (unsigned long long)atol(getenv("DEMCZ_PING_MS")) : 200ull;
        hipLaunchKernelGGL(peer_ping_kernel, dim3(1), dim3(64), 0, h->stream, own, pb, h->n_peers, h->rank, R, 0xC0FFEE0000000001ull,
                           ping_ms * 100000ull, d_res);
        unsigned int res[2] = {0, 0};
        if (hipGetLastError() != hipSuccess) rc = fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: ping launch failed");
        if (rc == DEMCZ_OK) rc = sync_stream(h, h->stream, "demcz_comm_init (first contact)");
        if (rc == DEMCZ_OK && hipMemcpy(res, d_res, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: download failed");
        h->ping_wait_us = (double)res[1] / 100.0;
        const bool can_live = rc == DEMCZ_OK && live_span(h) > 0;
        agree = (res[0] && can_live) ? 1u : 0u;
        if (getenv("DEMCZ_DEBUG_LIVE")) fprintf(stderr, "[demcz] rank %d: first contact %s after %.1f us, LIVE launches %s\n", h->rank, res[0] ? "ok" : "FAILED", h->ping_wait_us, can_live ? "possible" : "not possible");
    }
    if (rc == DEMCZ_OK && (hipMemcpyAsync(d_ok, &agree, sizeof(agree), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
                           ncclAllReduce(d_ok, d_ok, 1, ncclUint32, ncclMin, h->comm, h->stream) != ncclSuccess)) rc = fail(h, DEMCZ_ERR_COMM, "demcz_comm_init: reduction failed");
    if (rc == DEMCZ_OK) rc = sync_stream(h, h->stream, "demcz_comm_init (hand-off agreement)");
    unsigned int all_agree = 0u;
    if (rc == DEMCZ_OK && hipMemcpy(&all_agree, d_ok, sizeof(all_agree), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DEMCZ_ERR_HIP, "demcz_comm_init: download failed");
    cleanup();
    h->ping_ok = (rc == DEMCZ_OK && all_agree) ? 1 : 0;
    if (rc || !all_agree) {
        h->peer_mode = 0;
        live_release(h);
        close_all();
        return rc;
    }
    h->peer_fence = true;
    // a second communicator and stream for the monitoring R-hat of a finished slab (rhat_enqueue): its two small all-reduces then
    // run beside the next slab's launch instead of holding every rank's compute stream until all ranks have joined
    // (collective: every rank is here -- the agreement above was unanimous)
    if (!h->comm_stream) HIPCHK(h, stream_acquire(h->cfg.device_id, &h->comm_stream));
    if (!h->comm_side) NCCLCHK(h, ncclCommSplit(h->comm, 0, h->rank, &h->comm_side, nullptr));
    return DEMCZ_OK;
}

// The same set-up with the HOST carrying the handles (any transport: torch.distributed, MPI, Distributed.jl) and doing the two
// things a communicator does in mode 2: the ranks must meet (a barrier of the host's) between demcz_set_state and the first
// demcz_run, and between the last synchronising call and demcz_destroy; and a hand-off that timed out is an error on the rank
// that saw it (DEMCZ_ERR_STATE), not an automatic redo -- the ranks have no way here to agree on one.
extern "C" int32_t demcz_peer_export(demcz_handle* h, int32_t nranks, int32_t rank, void* handle_64B)
{
    NOT_DERIVED(h);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    if (!h || !handle_64B || nranks < 2 || nranks > DEMCZ_MAX_PEERS + 1 || rank < 0 || rank >= nranks) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->comm || h->peer_mode != 0) return fail(h, DEMCZ_ERR_STATE, "demcz_peer_export: handle is already sharded");
    if (!peer_capable(h)) return fail(h, DEMCZ_ERR_STATE, "demcz_peer_export: this layout has no in-launch hand-off");
    if (h->cfg.chain_id0 != (int64_t)rank * h->cfg.N) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_peer_export: chain_id0 must be rank * N");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->live_log.empty()) { int32_t rcv = live_verify(h); if (rcv) return rcv; }
    hipIpcMemHandle_t mh;
    bool ok = false;
    int32_t rc = archive_make_fine(h, &mh, &ok);
    if (rc) return rc;
    if (!ok) return fail(h, DEMCZ_ERR_HIP, "demcz_peer_export: fine-grained allocation or hipIpcGetMemHandle refused");
    std::memcpy(handle_64B, &mh, sizeof(mh));
    h->nranks = nranks;
    h->rank = rank;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_peer_attach(demcz_handle* h, const void* handles_64B_each)
{
    NOT_DERIVED(h);
    if (!h || !handles_64B_each) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->archive_fine || h->peer_mode != 0 || h->nranks < 2) return fail(h, DEMCZ_ERR_STATE, "demcz_peer_attach: call demcz_peer_export first");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    std::vector<hipIpcMemHandle_t> hs((size_t)h->nranks);
    std::memcpy(hs.data(), handles_64B_each, sizeof(hipIpcMemHandle_t) * (size_t)h->nranks);
    if (!peers_open(h, hs.data(), h->nranks, h->rank)) return fail(h, DEMCZ_ERR_HIP, "demcz_peer_attach: hipIpcOpenMemHandle refused (peer access between the devices?)");
    peer_no_dual(h);
    h->peer_mode = 3;
    rec_invalidate(h);
    return DEMCZ_OK;
}

// Mode 3, the orderly end: a rank's exported archive may only be freed once no other rank has it mapped.  The host makes the
// ranks meet after their last synchronising call, every rank calls demcz_peer_detach (its results stay readable, it runs no
// further generations), the host makes them meet once more, and only then does any rank call demcz_destroy.
extern "C" int32_t demcz_peer_detach(demcz_handle* h)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (h->peer_mode != 3) return fail(h, DEMCZ_ERR_STATE, "demcz_peer_detach: host-mediated IPC peers only (demcz_peer_export / demcz_peer_attach)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rc = live_verify(h);
    if (rc) return rc;
    for (hipStream_t st : {h->stream, h->prod_stream, h->diag_stream})
        if (st) HIPCHK(h, hipStreamSynchronize(st));
    for (int r = 0; r < DEMCZ_MAX_PEERS; ++r)
        if (h->ipc_mapped[r]) { (void)hipIpcCloseMemHandle(h->ipc_mapped[r]); h->ipc_mapped[r] = nullptr; }
    h->peers_closed = true;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_peer_ping(const demcz_handle* h, int32_t* ok, double* wait_us)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (ok) *ok = h->ping_ok;
    if (wait_us) *wait_us = h->ping_wait_us;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_comm_timeout(demcz_handle* h, int64_t milliseconds)
{
    NOT_DERIVED(h);
    if (!h || milliseconds < 0) return DEMCZ_ERR_INVALID_ARGUMENT;
    h->comm_timeout_ms = milliseconds;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_debug_stall_exchange(demcz_handle* h, int32_t milliseconds)
{
    NOT_DERIVED(h);
    if (!h || milliseconds < 0 || milliseconds > 10000) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->comm) return fail(h, DEMCZ_ERR_STATE, "demcz_debug_stall_exchange: not a sharded handle (demcz_comm_init)");
    h->stall_next_ms = milliseconds;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_export_current_device(demcz_handle* h, double* X_device)
{
    NOT_DERIVED(h);
    if (!h || !X_device) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_export_current_device: no state");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMemcpyAsync(X_device, h->dX, (size_t)h->cfg.N * h->cfg.d * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_append_rows_device(demcz_handle* h, const double* rows_device, int64_t nrows, int64_t ldrows)
{
    NOT_DERIVED(h);
    if (!h || !rows_device || nrows < 1 || ldrows < nrows) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_append_rows_device: no state");
    if (h->M_app + nrows > h->cfg.Mcap) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_append_rows_device: Z capacity exceeded");
    if (h->lag != 0) return fail(h, DEMCZ_ERR_STATE, "demcz_append_rows_device: caller-driven appends need append lag 0 on the handle");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int64_t tot = nrows * h->cfg.d;
    hipLaunchKernelGGL(append_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ, h->ZS, h->M_app,
                       rows_device, nrows, ldrows, h->cfg.d);
    HIPCHK(h, hipGetLastError());
    h->M_app += nrows;
    h->M = h->M_app;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_append_rows(demcz_handle* h, const double* rows, int64_t nrows, int64_t ldrows)
{
    NOT_DERIVED(h);
    if (!h || !rows || nrows < 1 || ldrows < nrows) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_append_rows: no state");
    if (h->M_app + nrows > h->cfg.Mcap) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_append_rows: Z capacity exceeded");
    if (h->lag != 0) return fail(h, DEMCZ_ERR_STATE, "demcz_append_rows: caller-driven appends need append lag 0 on the handle");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rcz = ensure_scratch(h, nrows * h->cfg.d);
    if (rcz) return rcz;
    HIPCHK(h, hipMemcpy2DAsync(h->d_scratch, (size_t)nrows * sizeof(double), rows, (size_t)ldrows * sizeof(double),
                               (size_t)nrows * sizeof(double), (size_t)h->cfg.d, hipMemcpyHostToDevice, h->stream));
    const int64_t tot = nrows * h->cfg.d;
    hipLaunchKernelGGL(append_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ, h->ZS, h->M_app,
                       (const double*)h->d_scratch, nrows, nrows, h->cfg.d);
    HIPCHK(h, hipGetLastError());
    SYNCCHK(h, h->stream);   // the caller may reuse `rows` on return
    h->M_app += nrows;
    h->M = h->M_app;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_external_append(demcz_handle* h, int32_t enabled)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->live_log.empty()) { int32_t rcv = live_verify(h); if (rcv) return rcv; }
    if (enabled && h->cr_adapt_every > 0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_external_append: the handle adapts its crossover weights (demcz_set_crossover_adapt) on its own "
                                        "chains: a shard's chains are not the population");
    h->external_append = enabled != 0;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_append_lag(demcz_handle* h, int32_t batches)
{
    NOT_DERIVED(h);
    if (!h || batches < 0 || batches > 64) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->live_log.empty()) { int32_t rcv = live_verify(h); if (rcv) return rcv; }
    if (h->M_app != h->M || !h->pending.empty()) return fail(h, DEMCZ_ERR_STATE, "demcz_set_append_lag: rows are still pending");
    if (h->external_append && batches) return fail(h, DEMCZ_ERR_STATE, "demcz_set_append_lag: caller-driven appends schedule their own visibility");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (h->comm && batches > 0) {
        // side stream + double-buffered batch slabs: [E][d][n_loc] out, [R][E][d][n_loc] in
        if (!h->comm_stream) HIPCHK(h, stream_acquire(h->cfg.device_id, &h->comm_stream));
        // a communicator of its own for the side stream (collective over the parent: every rank makes this call)
        // (nothing of the parent communicator may still be queued on the compute stream when it is split)
        SYNCCHK(h, h->stream);
        SYNCCHK(h, h->comm_stream);
        if (!h->comm_side) NCCLCHK(h, ncclCommSplit(h->comm, 0, h->rank, &h->comm_side, nullptr));
        const size_t one = (size_t)h->cfg.N * h->cfg.d * sizeof(double);
        for (int b = 0; b < 2; ++b) {
            if (h->d_send[b]) HIPCHK(h, dev_free(h->cfg.device_id, h->d_send[b]));
            if (h->d_recv[b]) HIPCHK(h, dev_free(h->cfg.device_id, h->d_recv[b]));
            h->d_send[b] = h->d_recv[b] = nullptr;
            HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_send[b], one * batches));
            HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_recv[b], one * batches * h->nranks));
            if (!h->buf_done[b]) {
                HIPCHK(h, hipEventCreateWithFlags(&h->buf_done[b], hipEventDisableTiming));
                HIPCHK(h, hipEventRecord(h->buf_done[b], h->comm_stream));
            }
        }
    }
    h->lag = batches;
    rec_invalidate(h);
    h->batch_cnt = 0; h->batch_buf = 0; h->batch_J = -1;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_rng_offset(demcz_handle* h, int64_t generations)
{
    NOT_DERIVED(h);
    if (!h || generations < 0) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->live_log.empty()) { int32_t rcv = live_verify(h); if (rcv) return rcv; }
    h->rng_offset = generations;
    rec_invalidate(h);
    return DEMCZ_OK;
}

// Snooker generations.  The choice of move is a fact of the generation, the same for all chains and
// known to the host: plan_launch cuts a snooker generation into a launch of its own and run_call launches snooker_kernel for it.
extern "C" int32_t demcz_set_snooker(demcz_handle* h, int32_t every, double gamma_lo, double gamma_hi)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (every < 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_snooker: every must be >= 0 (0 switches the snooker generations off)");
    if (!std::isfinite(gamma_lo) || !std::isfinite(gamma_hi) || !(0.0 < gamma_lo && gamma_lo <= gamma_hi))
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_snooker: the bounds of gamma_s must be finite with 0 < gamma_lo <= gamma_hi");
    if (h->cfg.target_kind == DEMCZ_TARGET_HOST_CALLBACK)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_snooker: a host-callback handle proposes through demcz_propose: it has no snooker generations");
    if (h->peer_mode != 0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_snooker: the handle is in a replica group or has IPC peers: their launches hand rows over "
                                        "inside them and are not cut at snooker generations");
    if (h->cfg.d < 2) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_snooker: the snooker step needs d >= 2 (a line through two points of a plane or more)");
    if (h->lanes != 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_snooker: the handle was not created on the one-lane layout (create it with "
                                                   "lanes_per_chain = 1): the other layouts draw ahead of the chains");
    h->snooker_every = every;
    h->snooker_lo = gamma_lo;
    h->snooker_hi = gamma_hi;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_snooker(const demcz_handle* h, int32_t* every, double* gamma_lo, double* gamma_hi, int64_t* steps_launched)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (every) *every = (int32_t)h->snooker_every;
    if (gamma_lo) *gamma_lo = h->snooker_lo;
    if (gamma_hi) *gamma_hi = h->snooker_hi;
    if (steps_launched) *steps_launched = h->snooker_steps;
    return DEMCZ_OK;
}

// the handle's weights (and their cumulative sums) into the adaptation's block on the device
static int32_t cr_adapt_upload_weights(demcz_handle* h)
{
    int32_t w[CR_MAX_CLASSES];
    uint32_t cum[CR_MAX_CLASSES];
    uint32_t sum = 0;
    for (int k = 0; k < CR_MAX_CLASSES; ++k) {
        w[k] = k < h->cr_ncr ? h->cr_weights[k] : 0;
        if (k < h->cr_ncr) sum += (uint32_t)h->cr_weights[k];
        cum[k] = sum;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMemcpyAsync(h->d_cr_adapt + CRA_WEIGHTS, w, sizeof w, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_cr_adapt + CRA_CUM, cum, sizeof cum, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DEMCZ_OK;
}

// Crossover generations.  The choices differ from chain to chain and are made inside the kernel;
// the host knows only that the handle's generations are crossover generations (window_kernel_of: ARM_CROSSOVER) and that a
// generation takes crossover_stride(d, delta_max) Philox blocks.
extern "C" int32_t demcz_set_crossover(demcz_handle* h, int32_t ncr, const int32_t* weights, int32_t delta_max)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (ncr < 0 || ncr > CR_MAX_CLASSES) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: ncr must be 0 (off) or 1 ... 8");
    if (delta_max < 1 || delta_max > CR_MAX_PAIRS) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: delta_max must be 1, 2 or 3");
    int64_t W = 0;
    for (int k = 0; k < ncr; ++k) {
        const int32_t wk = weights ? weights[k] : 1;
        if (wk < 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: a weight is negative");
        W += wk;
    }
    if (ncr > 0 && (W < 1 || W >= (int64_t)1 << 31))
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: the weights must sum to a W with 1 <= W < 2^31");
    if (h->cfg.target_kind == DEMCZ_TARGET_HOST_CALLBACK)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover: a host-callback handle proposes through demcz_propose: the closure mode has no crossover");
    if (h->peer_mode != 0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover: the handle is in a replica group or has IPC peers: crossover is not built for them");
    if (h->launches > 0 || h->g_done != h->g0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover: the handle has already run a generation: the stride of the Philox streams cannot "
                                        "change in mid-life (set crossover on the fresh handle, before demcz_set_rng_offset and demcz_run)");
    if (h->cfg.d < 2) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: crossover needs d >= 2");
    if (!h->full_block)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: the handle has more than one block (or not the block 0 .. d-1 in order): "
                                                   "crossover draws its own subsets and is not built for blocked handles");
    if (h->lanes != 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover: the handle was not created on the one-lane layout (create it with "
                                                   "lanes_per_chain = 1): the other layouts draw ahead of the chains");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (ncr > 0) {
        const size_t n = (size_t)((h->cfg.N + WINDOW_BS - 1) / WINDOW_BS) * 2 * CR_MAX_CLASSES;
        if (!h->d_cr_counts) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_cr_counts, n * sizeof(unsigned long long)));
        HIPCHK(h, hipMemsetAsync(h->d_cr_counts, 0, n * sizeof(unsigned long long), h->stream));
    }
    if (ncr == 0 || ncr != h->cr_ncr) { h->cr_adapt_every = 0; h->cr_adapt_until = 0; h->cr_adapt_started = false; }      // adaptation goes with its classes
    h->cr_ncr = ncr;
    h->cr_delta_max = delta_max;
    for (int k = 0; k < CR_MAX_CLASSES; ++k) h->cr_weights[k] = (k < ncr) ? (weights ? weights[k] : 1) : 1;
    h->S = ncr > 0 ? crossover_stride(h->cfg.d, delta_max) : h->S_plain;
    if (h->cr_adapt_every > 0) return cr_adapt_upload_weights(h);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_crossover(const demcz_handle* h, int32_t* ncr, int32_t* weights, int32_t* delta_max, int64_t* tried, int64_t* accepted)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (ncr) *ncr = h->cr_ncr;
    if (delta_max) *delta_max = h->cr_delta_max;
    if (weights) {
        for (int k = 0; k < h->cr_ncr; ++k) weights[k] = h->cr_weights[k];
        if (h->cr_adapt_every > 0 && h->cr_ncr > 0) {      // the device's: they change with no host in between
            demcz_handle* hm = const_cast<demcz_handle*>(h);
            int32_t dw[CR_MAX_CLASSES];
            HIPCHK(hm, hipSetDevice(h->cfg.device_id));
            HIPCHK(hm, hipMemcpyAsync(dw, h->d_cr_adapt + CRA_WEIGHTS, sizeof dw, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hm, hipStreamSynchronize(h->stream));
            for (int k = 0; k < h->cr_ncr; ++k) weights[k] = dw[k];
        }
    }
    if (tried || accepted) {
        demcz_handle* hm = const_cast<demcz_handle*>(h);
        int64_t sums[2 * CR_MAX_CLASSES] = {0};
        if (h->d_cr_counts && h->cr_ncr > 0) {
            // the workgroups' slots, summed on the host: a few kilobytes, on request only
            HIPCHK(hm, hipSetDevice(h->cfg.device_id));
            const size_t nwg = (size_t)((h->cfg.N + WINDOW_BS - 1) / WINDOW_BS);
            std::vector<unsigned long long> host(nwg * 2 * CR_MAX_CLASSES);
            HIPCHK(hm, hipMemcpyAsync(host.data(), h->d_cr_counts, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hm, hipStreamSynchronize(h->stream));
            for (size_t w = 0; w < nwg; ++w)
                for (int i = 0; i < 2 * CR_MAX_CLASSES; ++i) sums[i] += (int64_t)host[w * 2 * CR_MAX_CLASSES + i];
        }
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            if (tried) tried[k] = sums[2 * k];
            if (accepted) accepted[k] = sums[2 * k + 1];
        }
    }
    return DEMCZ_OK;
}

// Adaptation of the class weights during burn-in.  The host knows the positions (plan_launch cuts a
// launch at every update position up to `until`) and enqueues cr_adapt_kernel behind such a launch; what is adapted on, and the
// weights themselves, stay on the device.
extern "C" int32_t demcz_set_crossover_adapt(demcz_handle* h, int64_t every, int64_t until, int32_t min_weight)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (every < 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt: every must be >= 0 (0 switches the adaptation off)");
    if (every == 0) {
        // (a handle that runs the ADAPT kernels keeps them for life)
        if (h->cr_adapt_every > 0 && (h->launches > 0 || h->g_done != h->g0))
            return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt: the handle has already run a generation: the adaptation is switched off on the "
                                            "fresh handle only (behind `until` it has ended by itself)");
        h->cr_adapt_every = 0; h->cr_adapt_until = 0; h->cr_adapt_started = false;
        return DEMCZ_OK;
    }
    if (until < every || until % every != 0)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt: until must be a multiple of every, and at least every");
    if (min_weight < 1 || min_weight > 8192)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt: min_weight must be 1 ... 8192 (of 65536)");
    // a step adds at most 2^32 to a class's distance
    if (until >= ((int64_t)1 << 31) || (__int128)h->cfg.N * (__int128)until >= ((__int128)1 << 31))
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt: N * until must stay below 2^31 (the distance sums are 64-bit integers)");
    if (h->cr_ncr == 0) return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt: the handle has no crossover generations (demcz_set_crossover first)");
    if (h->launches > 0 || h->g_done != h->g0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt: the handle has already run a generation (set the adaptation on the fresh handle; "
                                        "demcz_set_crossover_weights changes the weights of a running one)");
    if (h->external_append)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt: the handle appends externally (demcz_set_external_append): a shard's own chains are "
                                        "not the population (demcz_set_crossover_weights sets a shard's weights by hand)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->d_cr_adapt) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_cr_adapt, cra_bytes(h)));
    HIPCHK(h, hipMemsetAsync(h->d_cr_adapt, 0, cra_bytes(h), h->stream));
    h->cr_adapt_every = every;
    h->cr_adapt_until = until;
    h->cr_adapt_min_weight = min_weight;
    h->cr_adapt_started = false;
    return cr_adapt_upload_weights(h);
}

extern "C" int32_t demcz_get_crossover_adapt(const demcz_handle* h, int64_t* every, int64_t* until, int32_t* min_weight, int32_t* weights,
                                             int64_t* dist, int64_t* tried, double* rsd, int64_t* updates)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (every) *every = h->cr_adapt_every;
    if (until) *until = h->cr_adapt_until;
    if (min_weight) *min_weight = h->cr_adapt_min_weight;
    if (h->cr_adapt_every == 0) {
        if (updates) *updates = 0;
        for (int k = 0; k < CR_MAX_CLASSES; ++k) {
            if (weights) weights[k] = k < h->cr_ncr ? h->cr_weights[k] : 0;
            if (dist) dist[k] = 0;
            if (tried) tried[k] = 0;
        }
        if (rsd) for (int p = 0; p < h->cfg.d; ++p) rsd[p] = 0.0;
        return DEMCZ_OK;
    }
    demcz_handle* hm = const_cast<demcz_handle*>(h);
    HIPCHK(hm, hipSetDevice(h->cfg.device_id));
    std::vector<unsigned char> host(cra_bytes(h));
    HIPCHK(hm, hipMemcpyAsync(host.data(), h->d_cr_adapt, host.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hm, hipStreamSynchronize(h->stream));
    unsigned long long sums[2 * CR_MAX_CLASSES] = {0};
    for (size_t w = 0; w < cra_workgroups(h); ++w)
        for (int i = 0; i < 2 * CR_MAX_CLASSES; ++i) {
            unsigned long long v;
            memcpy(&v, host.data() + CRA_SLOTS + (w * 2 * CR_MAX_CLASSES + i) * sizeof v, sizeof v);
            sums[i] += v;
        }
    for (int k = 0; k < CR_MAX_CLASSES; ++k) {
        if (weights) memcpy(&weights[k], host.data() + CRA_WEIGHTS + 4 * k, 4);
        if (dist) dist[k] = (int64_t)sums[2 * k];
        if (tried) tried[k] = (int64_t)sums[2 * k + 1];
    }
    if (rsd) memcpy(rsd, host.data() + CRA_RSD, sizeof(double) * (size_t)h->cfg.d);
    if (updates) memcpy(updates, host.data() + CRA_UPDATES, sizeof(int64_t));
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_crossover_adapt_state(demcz_handle* h, const int32_t* weights, int64_t* dist, int64_t* tried,
                                                   const double* rsd, int64_t updates)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (h->cr_adapt_every == 0) return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt_state: the handle has no adaptation set (demcz_set_crossover_adapt first)");
    if (h->launches > 0 || h->g_done != h->g0)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_adapt_state: the handle has already run a generation: the state of a checkpoint goes "
                                        "onto the fresh handle");
    if (!weights || !dist || !tried || !rsd || updates < 0)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt_state: weights, dist, tried and rsd are required, updates >= 0");
    int64_t W = 0;
    for (int k = 0; k < h->cr_ncr; ++k) {
        if (weights[k] < 0 || dist[k] < 0 || tried[k] < 0)
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt_state: a weight, a distance or a count is negative");
        W += weights[k];
    }
    if (W < 1 || W >= (int64_t)1 << 31)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_adapt_state: the weights must sum to a W with 1 <= W < 2^31");
    std::vector<unsigned char> host(cra_bytes(h), 0);
    for (int k = 0; k < h->cr_ncr; ++k) {
        h->cr_weights[k] = weights[k];
        const unsigned long long dv = (unsigned long long)dist[k], tv = (unsigned long long)tried[k];
        memcpy(host.data() + CRA_SLOTS + (2 * k) * sizeof dv, &dv, sizeof dv);            // workgroup 0's slots hold the totals
        memcpy(host.data() + CRA_SLOTS + (2 * k + 1) * sizeof tv, &tv, sizeof tv);
    }
    memcpy(host.data() + CRA_UPDATES, &updates, sizeof updates);
    memcpy(host.data() + CRA_RSD, rsd, sizeof(double) * (size_t)h->cfg.d);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMemcpyAsync(h->d_cr_adapt, host.data(), host.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->cr_adapt_started = true;       // the spread is the checkpoint's
    return cr_adapt_upload_weights(h);
}

extern "C" int32_t demcz_set_crossover_weights(demcz_handle* h, const int32_t* weights)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (h->cr_ncr == 0) return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_weights: the handle has no crossover generations (demcz_set_crossover)");
    if (!weights) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_weights: weights is required");
    int64_t W = 0;
    for (int k = 0; k < h->cr_ncr; ++k) {
        if (weights[k] < 0) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_weights: a weight is negative");
        W += weights[k];
    }
    if (W < 1 || W >= (int64_t)1 << 31)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_set_crossover_weights: the weights must sum to a W with 1 <= W < 2^31");
    // (updates * every < until, said in positions: the update on `until` is the last)
    if (h->cr_adapt_every > 0 && h->g_done + h->rng_offset < h->cr_adapt_until)
        return fail(h, DEMCZ_ERR_STATE, "demcz_set_crossover_weights: the adaptation is still running (it sets the weights until the generation "
                                        "`until` of demcz_set_crossover_adapt has run)");
    for (int k = 0; k < h->cr_ncr; ++k) h->cr_weights[k] = weights[k];
    if (h->cr_adapt_every > 0) return cr_adapt_upload_weights(h);       // (stream-ordered behind the launches that read the old ones)
    return DEMCZ_OK;
}

// ---- stateless diagnostics on caller arrays (src/utils.jl) ------------------------------------------
namespace {
// A demcz_handle that only holds a history: the caller's host arrays, uploaded for the length of one _array call into hipMalloc
// blocks of their own, behind a stream created for the call.  derived_create (below) is the other builder of such a handle: a
// history that outlives the call that made it, from the pools.  They stay two because merging them would move one's memory to
// where the other's comes from.
struct ScratchHandle {
    demcz_handle h;
    int32_t open(int32_t device_id, int64_t N, int d, int64_t G, const double* chain, const double* log_obj)
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, DEMCZ_ERR_NO_DEVICE, "no HIP device visible (there is no CPU fallback)");
        if (device_id < 0 || device_id >= ndev || N < 1 || d < 1 || G < 1) return fail(nullptr, DEMCZ_ERR_INVALID_ARGUMENT, "bad device or shape");
        h.cfg.N = N; h.cfg.d = d; h.cfg.Gcap = G; h.cfg.device_id = device_id; h.g0 = 0; h.nranks = 1;
        HIPCHK(&h, hipSetDevice(device_id));
        HIPCHK(&h, hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
        h.own_stream = true;
        if (chain) {
            HIPCHK(&h, hipMalloc((void**)&h.dchain, (size_t)N * d * G * sizeof(double)));
            HIPCHK(&h, hipMemcpyAsync(h.dchain, chain, (size_t)N * d * G * sizeof(double), hipMemcpyHostToDevice, h.stream));
        }
        if (log_obj) {
            HIPCHK(&h, hipMalloc((void**)&h.dlogobj, (size_t)N * G * sizeof(double)));
            HIPCHK(&h, hipMemcpyAsync(h.dlogobj, log_obj, (size_t)N * G * sizeof(double), hipMemcpyHostToDevice, h.stream));
        }
        h.stage_cap = 4096 + (int64_t)d * (d + 1);
        HIPCHK(&h, hipHostMalloc((void**)&h.d_stage, (size_t)h.stage_cap * sizeof(double), hipHostMallocDefault));
        return DEMCZ_OK;
    }
    ~ScratchHandle()
    {
        if (h.stream) (void)hipStreamSynchronize(h.stream);
        free_all(&h);
    }
};
int32_t diag_fail(const ScratchHandle& s, int32_t rc)
{
    if (rc) g_create_error = s.h.err;
    return rc;
}

// The body of every _array entry point: the arrays go up into a ScratchHandle, fn works on it as on any handle holding generations
// 1..G, the uploads are freed when the call returns, and a failure's message moves to where demcz_last_error(NULL) finds it.
template <class F>
int32_t with_arrays(int32_t device_id, int64_t N, int d, int64_t G, const double* chain, const double* log_obj, F fn)
{
    ScratchHandle s;
    int32_t rc = s.open(device_id, N, d, G, chain, log_obj);
    return diag_fail(s, rc ? rc : fn(&s.h));
}
}  // namespace

extern "C" int32_t demcz_rhat_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, double* rhat)
{
    if (!chain || !rhat) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return demcz_rhat(h, 1, G, rhat); });
}

extern "C" int32_t demcz_autocov_sums_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G,
                                            int64_t lag_from, int64_t lag_to, double* sums)
{
    if (!chain || !sums) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return demcz_autocov_sums(h, 1, G, lag_from, lag_to, sums); });
}

extern "C" int32_t demcz_ess_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t max_lag,
                                   double* ess, double* tau, double* varplus, int64_t* pairs, int32_t* converged)
{
    if (!chain || !ess) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr,
                       [&](demcz_handle* h) { return demcz_ess(h, 1, G, max_lag, ess, tau, varplus, pairs, converged); });
}

extern "C" int32_t demcz_quantiles_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nq,
                                         const double* probs, double* q, double* lower, double* upper)
{
    if (!chain || !probs || !q) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return demcz_quantiles(h, 1, G, nq, probs, q, lower, upper); });
}

extern "C" int32_t demcz_best_array(int32_t device_id, const double* log_obj, int64_t N, int64_t G, double* bestval, int64_t* chain,
                                    int64_t* column)
{
    if (!log_obj || !bestval || !chain || !column) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, 1, G, nullptr, log_obj, [&](demcz_handle* h) {
        int64_t g = -1;
        int32_t rc = demcz_best(h, 1, G, bestval, chain, &g, nullptr);
        if (!rc) *column = (g < 0) ? -1 : g - 1;
        return rc;
    });
}

extern "C" int32_t demcz_accept_ratio_array(int32_t device_id, const double* log_obj, int64_t N, int64_t G, double* ratio)
{
    if (!log_obj || !ratio) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, 1, G, nullptr, log_obj, [&](demcz_handle* h) { return demcz_accept_ratio(h, 1, G, ratio); });
}

extern "C" int32_t demcz_mean_cov_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, double* mean, double* cov)
{
    if (!chain || !mean || !cov) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return demcz_mean_cov(h, 1, G, mean, cov); });
}

// ---- derived quantities: user functions of the draws (demcz_kernels_derive.h) -----------------------------------------------
extern "C" int32_t demcz_derive_check(int32_t d, int32_t m, const char* source, const char* options)
{
    return program_compile(nullptr, demcz_prog::UNIT_DERIVE, d, m, source, options);
}

namespace {
// ---- what the workers on a window of a history share (derive, rank, pointwise, loo, bridge) --------------------------------------
// A launch or a synchronisation that failed with DEMCZ_ERR_HIP says nothing about the kernels queued before it: the device is
// synchronised before anything they may still be writing is released.  The one home of that rule: a worker passes the status of
// its device work through here while the owners of what its kernels write (NewDerived, DevBlock) are still in scope.
int32_t settle(int32_t rc)
{
    if (rc == DEMCZ_ERR_HIP) (void)hipDeviceSynchronize();
    return rc;
}

// A derived history between derived_create and its hand-over to the caller (release()).  A producer that fails on the way frees
// it with free_all: only the producer knows it, and nothing has been queued on its stream since derived_create waited for it.
struct FreeDerived {
    void operator()(demcz_handle* dh) const { free_all(dh); delete dh; }
};
using NewDerived = std::unique_ptr<demcz_handle, FreeDerived>;

// A complete derived history that a worker had a producer make, to take statistics of it and drop it: dropped as its user would,
// with demcz_destroy, which waits for the history's own stream (the statistics ran there) before the buffers go back to the pools.
// (Not a unique_ptr: the producers fill a demcz_handle**, as the entry points need it.)
struct Part {
    demcz_handle* h = nullptr;
    Part() = default;
    Part(const Part&) = delete;
    Part& operator=(const Part&) = delete;
    ~Part() { (void)demcz_destroy(h); }
};

// the status of a call on another handle than the caller's (a Part, the second history of a pair): its error message moves to
// the handle the caller holds
int32_t part_rc(demcz_handle* caller, const demcz_handle* part, int32_t rc)
{
    if (rc) caller->err = part->err;
    return rc;
}

// A dev_malloc block that goes back to the pool when its scope ends (after settle(), if kernels were given it)
struct DevBlock {
    int device = 0;
    void* p = nullptr;
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    ~DevBlock() { (void)dev_free(device, p); }
    hipError_t alloc(int dev, size_t bytes)
    {
        device = dev;
        const hipError_t e = dev_malloc(dev, &p, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
        return e;
    }
};

// The window g_from..g_to of h's history as the kernels index it: N chains, d columns, w generations from slot s0, total = N w
struct Window {
    int64_t N, w, s0, total;
    int d;
};

// A worker's first stage: the range check, whose refusal names `who`, and the window.  Its own argument checks come next.
int32_t open_window(demcz_handle* h, int64_t g_from, int64_t g_to, const char* who, Window& win)
{
    int32_t rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    win.N = h->cfg.N; win.d = h->cfg.d; win.w = g_to - g_from + 1; win.s0 = g_from - h->g0 - 1; win.total = win.N * win.w;
    return DEMCZ_OK;
}

// ... and its second, behind those checks: h's device is current and what h's launches wrote is verified.  (quiesce_all stays the
// worker's own line, right before its first allocation: some compile a program or check a size in between.)
int32_t enter_device(demcz_handle* h)
{
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    return live_verify(h);
}

// A producer's last stage, `launched` being what its one launch returned: a failed launch goes to h->err, otherwise h's stream is
// waited for.  Then the history is the caller's; on a failure it stays with its owner, which frees it behind the settling here.
int32_t finish(demcz_handle* h, const char* who, const char* kernel, hipError_t launched, NewDerived& dh, demcz_handle** out)
{
    int32_t rc = DEMCZ_ERR_HIP;
    if (launched != hipSuccess) h->err = std::string(who) + ": launching " + kernel + ": " + hipGetErrorString(launched);
    else rc = sync_stream(h, h->stream, who);
    if (!rc) *out = dh.release();
    return settle(rc);
}

// The derived history of N x m x w values on `device`, generations g0 + 1 .. g0 + w, with `data` copied into memory it owns:
// a handle on the heap that outlives the call that makes it, its buffers and its stream from the pools.  ScratchHandle (above) is
// the other builder of a handle that only holds a history: an _array call's uploads in hipMalloc blocks of their own, gone when
// the call returns; they stay two so that neither's memory moves to where the other's comes from.  On failure everything made so
// far is freed, null is returned and `why` says what failed.
NewDerived derived_create(int device, int64_t N, int m, int64_t w, int64_t g0, const double* data, int64_t ndata, std::string& why,
                          const char* who = "demcz_derive")
{
    NewDerived dh(new demcz_handle);
    dh->cfg.N = N; dh->cfg.d = m; dh->cfg.Gcap = w; dh->cfg.device_id = device; dh->cfg.nobs = ndata;
    dh->g0 = g0; dh->nranks = 1; dh->derived = true;
    dh->stage_cap = 4096 + (int64_t)m * (m + 1);
    const char* what = "hipSetDevice";
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) { what = "the derived history's stream"; e = stream_acquire(device, &dh->stream); dh->own_stream = e == hipSuccess; }
    if (e == hipSuccess) { what = "the derived history (N x m x w doubles)"; e = dev_malloc(device, (void**)&dh->dchain, (size_t)N * m * w * sizeof(double)); }
    if (e == hipSuccess) { what = "the program's data"; e = dev_alloc_copy(&dh->d_design, data, (size_t)ndata, dh->stream, device); }
    if (e == hipSuccess) { what = "the staging buffer"; e = host_malloc((void**)&dh->d_stage, (size_t)dh->stage_cap * sizeof(double)); }
    if (e == hipSuccess) { what = "the upload of the program's data"; e = hipStreamSynchronize(dh->stream); }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        why = std::string(who) + ": " + what + ": " + hipGetErrorString(e);
        return nullptr;
    }
    return dh;
}

unsigned derive_blocks(int64_t total) { return (unsigned)std::min<int64_t>((total + DERIVE_THREADS - 1) / DERIVE_THREADS, DERIVE_MAX_WG); }

// demcz_derive on a source that holds an N x d x Gcap history (a sampling handle, a derived history, a ScratchHandle)
int32_t derive_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                    const double* data, int64_t ndata, demcz_handle** derived)
{
    const char* who = "demcz_derive";
    Window win;
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    rc = data_check(h, who, data, ndata);
    if (rc) return rc;
    rc = enter_device(h);
    if (rc) return rc;
    demcz_prog::Module mod;
    rc = program_load(h, demcz_prog::UNIT_DERIVE, win.d, m, source, options, mod);
    if (rc) return rc;
    rc = quiesce_all(h);                        // (a sharded handle: the allocations below synchronise the device)
    if (rc) return rc;
    std::string err;
    NewDerived dh = derived_create(h->cfg.device_id, win.N, m, win.w, g_from - 1, data, ndata, err);
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    const double* chain = h->dchain;
    const double* logobj = h->dlogobj;          // (nullptr on a derived history and on arrays given without log_obj: logp is NaN)
    const double* ddata = ndata > 0 ? dh->d_design : nullptr;
    double* out = dh->dchain;
    void* args[] = {&chain, &logobj, &win.N, &win.s0, &win.total, &ddata, &ndata, &out};
    // on the source's stream: behind the window launches that write the history, and behind whatever else is queued there
    const hipError_t e = hipModuleLaunchKernel(mod.fn[demcz_prog::DERIVE_KERNEL], derive_blocks(win.total), 1, 1, DERIVE_THREADS, 1, 1, 0, h->stream, args, nullptr);
    return finish(h, who, "derive_kernel", e, dh, derived);
}
}  // namespace

extern "C" int32_t demcz_derive(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                                const double* data, int64_t ndata, demcz_handle** derived)
{
    if (!h || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    DEADCHK(h);
    return derive_from(h, g_from, g_to, m, source, options, data, ndata, derived);
}

extern "C" int32_t demcz_derive_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d, int64_t G,
                                      int32_t m, const char* source, const char* options, const double* data, int64_t ndata,
                                      demcz_handle** derived)
{
    if (!chain || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    // (compiled before anything is uploaded: a program that does not compile costs no copy)
    int32_t rc = demcz_derive_check(d, m, source, options);
    if (rc) return rc;
    // (the uploads are freed when this call returns: only the derived history stays)
    return with_arrays(device_id, N, d, G, chain, log_obj,
                       [&](demcz_handle* h) { return derive_from(h, 1, G, m, source, options, data, ndata, derived); });
}

// ---- posterior predictive programs: functions of the draws and of each draw's own random stream (demcz_kernels_predict.h) -------
extern "C" int32_t demcz_predict_check(int32_t d, int32_t m, const char* source, const char* options)
{
    return program_compile(nullptr, demcz_prog::UNIT_PREDICT, d, m, source, options);
}

namespace {
// What demcz_predict and demcz_ppc share up to their allocations: the window, the arguments, the stream's two 32-bit halves
// (generation and global chain: DESIGN.md section 3), the device, the program's module.
int32_t predict_open(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options, const double* data,
                     int64_t ndata, int64_t chain_id0, const char* who, Window& win, demcz_prog::Module& mod)
{
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    rc = data_check(h, who, data, ndata);
    if (rc) return rc;
    constexpr int64_t TWO32 = (int64_t)1 << 32;
    if (g_to >= TWO32 || chain_id0 < 0 || chain_id0 > TWO32 - win.N)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": the stream of a draw is keyed by (generation, global chain), 32 bits each: need "
                                                   "g_to < 2^32 and 0 <= chain_id0, chain_id0 + N <= 2^32");
    rc = enter_device(h);
    if (rc) return rc;
    rc = program_load(h, demcz_prog::UNIT_PREDICT, win.d, m, source, options, mod);
    if (rc) return rc;
    return quiesce_all(h);                     // (a sharded handle: the allocations that follow synchronise the device)
}

// demcz_predict on a source that holds an N x d x Gcap history (a sampling handle, a derived history, a ScratchHandle)
int32_t predict_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                     const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, demcz_handle** derived)
{
    const char* who = "demcz_predict";
    Window win;
    demcz_prog::Module mod;
    int32_t rc = predict_open(h, g_from, g_to, m, source, options, data, ndata, chain_id0, who, win, mod);
    if (rc) return rc;
    std::string err;
    NewDerived dh = derived_create(h->cfg.device_id, win.N, m, win.w, g_from - 1, data, ndata, err, who);
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    const double* chain = h->dchain;
    const double* logobj = h->dlogobj;          // (nullptr on a derived history and on arrays given without log_obj: logp is NaN)
    const double* ddata = ndata > 0 ? dh->d_design : nullptr;
    double* out = dh->dchain;
    void* args[] = {&chain, &logobj, &win.N, &win.s0, &win.total, &ddata, &ndata, &seed, &g_from, &chain_id0, &out};
    const hipError_t e = hipModuleLaunchKernel(mod.fn[demcz_prog::PREDICT_KERNEL], derive_blocks(win.total), 1, 1, DERIVE_THREADS, 1, 1, 0, h->stream, args, nullptr);
    return finish(h, who, "predict_kernel", e, dh, derived);
}

// demcz_ppc on such a source.  One pool block holds what the kernel reads and writes besides the history: the 3 m counters,
// observed, the program's data.
int32_t ppc_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options, const double* data,
                 int64_t ndata, uint64_t seed, int64_t chain_id0, const double* observed, int64_t* counts)
{
    const char* who = "demcz_ppc";
    Window win;
    demcz_prog::Module mod;
    int32_t rc = predict_open(h, g_from, g_to, m, source, options, data, ndata, chain_id0, who, win, mod);
    if (rc) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(double) && sizeof(int64_t) == sizeof(double), "one block of 8-byte words");
    const size_t nc = 3 * (size_t)m;
    std::vector<double> up((size_t)m + (size_t)ndata, 0.0);         // observed (NULL: zeros), then data
    if (observed) std::copy(observed, observed + m, up.begin());
    if (ndata > 0) std::copy(data, data + ndata, up.begin() + m);
    std::vector<int64_t> hc(nc);
    DevBlock blk;
    if (blk.alloc(h->cfg.device_id, (nc + up.size()) * sizeof(double)) != hipSuccess)
        return fail(h, DEMCZ_ERR_HIP, std::string(who) + ": the counters, observed and the program's data: out of device memory");
    unsigned long long* dcounts = static_cast<unsigned long long*>(blk.p);
    const double* dobs = reinterpret_cast<const double*>(dcounts + nc);
    const double* ddata = ndata > 0 ? dobs + m : nullptr;
    auto body = [&]() -> int32_t {
        HIPCHK(h, hipMemsetAsync(dcounts, 0, nc * sizeof(unsigned long long), h->stream));
        HIPCHK(h, hipMemcpyAsync(const_cast<double*>(dobs), up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const double* chain = h->dchain;
        const double* logobj = h->dlogobj;
        void* args[] = {&chain, &logobj, &win.N, &win.s0, &win.total, &ddata, &ndata, &seed, &g_from, &chain_id0, &dobs, &dcounts};
        const hipError_t e = hipModuleLaunchKernel(mod.fn[demcz_prog::PREDICT_PPC], derive_blocks(win.total), 1, 1, DERIVE_THREADS, 1, 1, 0, h->stream, args, nullptr);
        if (e != hipSuccess) return fail(h, DEMCZ_ERR_HIP, std::string(who) + ": launching ppc_kernel: " + hipGetErrorString(e));
        HIPCHK(h, hipMemcpyAsync(hc.data(), dcounts, nc * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        return sync_stream(h, h->stream, who);
    };
    rc = body();
    if (rc) { (void)hipStreamSynchronize(h->stream); return settle(rc); }   // (copies from and into this call's vectors may be under way)
    std::copy(hc.begin(), hc.end(), counts);
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_predict(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                                 const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, demcz_handle** derived)
{
    if (!h || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    DEADCHK(h);
    return predict_from(h, g_from, g_to, m, source, options, data, ndata, seed, chain_id0, derived);
}

extern "C" int32_t demcz_predict_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d, int64_t G,
                                       int32_t m, const char* source, const char* options, const double* data, int64_t ndata,
                                       uint64_t seed, int64_t chain_id0, demcz_handle** derived)
{
    if (!chain || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    // (compiled before anything is uploaded: a program that does not compile costs no copy)
    int32_t rc = demcz_predict_check(d, m, source, options);
    if (rc) return rc;
    return with_arrays(device_id, N, d, G, chain, log_obj,
                       [&](demcz_handle* h) { return predict_from(h, 1, G, m, source, options, data, ndata, seed, chain_id0, derived); });
}

extern "C" int32_t demcz_ppc(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t m, const char* source, const char* options,
                             const double* data, int64_t ndata, uint64_t seed, int64_t chain_id0, const double* observed, int64_t* counts)
{
    if (!h || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return ppc_from(h, g_from, g_to, m, source, options, data, ndata, seed, chain_id0, observed, counts);
}

extern "C" int32_t demcz_ppc_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d, int64_t G,
                                   int32_t m, const char* source, const char* options, const double* data, int64_t ndata,
                                   uint64_t seed, int64_t chain_id0, const double* observed, int64_t* counts)
{
    if (!chain || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = demcz_predict_check(d, m, source, options);
    if (rc) return rc;
    return with_arrays(device_id, N, d, G, chain, log_obj,
                       [&](demcz_handle* h) { return ppc_from(h, 1, G, m, source, options, data, ndata, seed, chain_id0, observed, counts); });
}

// ---- rank-normalised diagnostics (K10, demcz_kernels_rank.h): average ranks, normal scores, indicator columns -----------------
namespace {
// Everything a ranking needs besides the two key buffers, carved from ONE pool allocation so that there is one thing to free.
struct RankScratch {
    DevBlock base;
    uint64_t *buf0, *buf1;
    unsigned long long *hist, *nan;
    unsigned int* tcount;
    int* info;                      // [RANK_DIGITS + 1][d]: per pass the source buffer of each parameter or -1; last row: where it ends
    unsigned int* dbase;            // [RANK_DIGITS][d][256]: keys of the parameter with a smaller digit in that pass
    double* center;
    void* extra;                    // what the caller asked for besides (demcz_hdi: its partials and its result), 8-byte aligned
};

int32_t rank_refuse_sharded(demcz_handle* h, const char* who)
{
    if (h->comm && h->nranks > 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": a rank needs the draws of every shard: gather the window with "
                                                   "demcz_get_history on every rank and use the _array form on the whole");
    return DEMCZ_OK;
}

// The keys-only sort of the d columns of a window, shared by demcz_rank_normalize, demcz_loo_columns and demcz_hdi: the scratch and the host
// copies that have to live until the stream is synchronised.
struct RankSort {
    RankScratch sc;
    int64_t ntiles = 0;
    size_t nhist = 0, ninfo = 0;
    const double* dcenter = nullptr;            // sc.center once the centres are uploaded, else null
    std::vector<double> hcenter;
    std::vector<unsigned long long> hhist;
    std::vector<int> hinfo;
    std::vector<unsigned int> hbase;
};

// the scratch layout of a sort of d columns of S keys, and `extra` bytes behind it; freed with rs
int32_t rank_sort_alloc(demcz_handle* h, int d, int64_t S, const char* who, RankSort& rs, size_t extra = 0)
{
    RankScratch& sc = rs.sc;
    const int64_t ntiles = rs.ntiles = (S + RANK_TILE - 1) / RANK_TILE;
    // [buf0 | buf1 | hist | nan | center | tcount | dbase | info | extra], every piece a multiple of 8 bytes
    const size_t nkeys = (size_t)d * S, nhist = (size_t)d * RANK_DIGITS * 256, ntc = (size_t)d * ntiles * 256,
                 ninfo = (size_t)(RANK_DIGITS + 1) * d;
    const size_t bytes = 2 * nkeys * 8 + nhist * 8 + (size_t)d * 8 + (size_t)d * 8 + (ntc * 4 + 7) / 8 * 8 + nhist * 4 + (ninfo * 4 + 7) / 8 * 8;
    const hipError_t e = sc.base.alloc(h->cfg.device_id, bytes + extra);
    if (e != hipSuccess)
        return fail(h, DEMCZ_ERR_HIP, std::string(who) + ": the sort's scratch (two key buffers of N w d words): " + hipGetErrorString(e));
    sc.buf0 = static_cast<uint64_t*>(sc.base.p);
    sc.buf1 = sc.buf0 + nkeys;
    sc.hist = reinterpret_cast<unsigned long long*>(sc.buf1 + nkeys);
    sc.nan = sc.hist + nhist;
    sc.center = reinterpret_cast<double*>(sc.nan + d);
    sc.tcount = reinterpret_cast<unsigned int*>(sc.center + d);
    sc.dbase = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(sc.tcount) + (ntc * 4 + 7) / 8 * 8);
    sc.info = reinterpret_cast<int*>(sc.dbase + nhist);              // (nhist = d * 8 * 256 is even)
    sc.extra = static_cast<char*>(sc.base.p) + bytes;
    rs.nhist = nhist;
    rs.ninfo = ninfo;
    rs.hhist.assign(nhist, 0ull);
    rs.hinfo.assign(ninfo, -1);
    rs.hbase.assign(nhist, 0u);
    return DEMCZ_OK;
}

// keys, histograms, the host's sit-out table and the eight passes, queued on h's stream (which is synchronised once, for the
// histograms).  Afterwards column p's keys stand ascending in buf0 or buf1 as sc.info's last row says, its NaN count in sc.nan.
int32_t rank_sort_run(demcz_handle* h, int64_t N, int d, int64_t s0, int64_t S, const double* center, const char* who, RankSort& rs)
{
    RankScratch& sc = rs.sc;
    const int64_t ntiles = rs.ntiles;
    const size_t nhist = rs.nhist, ninfo = rs.ninfo;
    std::vector<unsigned long long>& hhist = rs.hhist;
    std::vector<int>& hinfo = rs.hinfo;
    std::vector<unsigned int>& hbase = rs.hbase;
    const double* dcenter = nullptr;
    if (center) {
        rs.hcenter.assign(center, center + d);
        HIPCHK(h, hipMemcpyAsync(sc.center, rs.hcenter.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, h->stream));
        dcenter = sc.center;
    }
    rs.dcenter = dcenter;
    HIPCHK(h, hipMemsetAsync(sc.hist, 0, (nhist + d) * sizeof(unsigned long long), h->stream));
    const dim3 grid((unsigned)ntiles, (unsigned)d);
    hipLaunchKernelGGL(rank_keys_kernel, grid, dim3(RANK_BS), 0, h->stream, (const double*)h->dchain, N, d, s0, S, dcenter, sc.buf0,
                       sc.hist, sc.nan);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hhist.data(), sc.hist, nhist * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    int32_t r2 = sync_stream(h, h->stream, who);
    if (r2) return r2;
    // a digit in which all S keys of a parameter agree leaves their order as it is: that parameter sits the pass out
    std::vector<int> cur((size_t)d, 0);
    bool any[RANK_DIGITS] = {};
    for (int b = 0; b < RANK_DIGITS; ++b)
        for (int p = 0; p < d; ++p) {
            const unsigned long long* hp = hhist.data() + ((size_t)p * RANK_DIGITS + b) * 256;
            unsigned int* bp = hbase.data() + ((size_t)b * d + p) * 256;
            bool one_bin = false;
            unsigned long long below = 0;
            for (int k = 0; k < 256; ++k) {
                one_bin = one_bin || hp[k] == (unsigned long long)S;
                bp[k] = (unsigned int)below;
                below += hp[k];
            }
            if (one_bin) continue;
            hinfo[(size_t)b * d + p] = cur[p];
            cur[p] ^= 1;
            any[b] = true;
        }
    for (int p = 0; p < d; ++p) hinfo[(size_t)RANK_DIGITS * d + p] = cur[p];
    HIPCHK(h, hipMemcpyAsync(sc.info, hinfo.data(), ninfo * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(sc.dbase, hbase.data(), nhist * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
    for (int b = 0; b < RANK_DIGITS; ++b) {
        if (!any[b]) continue;
        const int* info = sc.info + (size_t)b * d;
        hipLaunchKernelGGL(rank_tile_count_kernel, grid, dim3(RANK_BS), 0, h->stream, (const uint64_t*)sc.buf0, (const uint64_t*)sc.buf1,
                           S, ntiles, 8 * b, info, sc.tcount);
        hipLaunchKernelGGL(rank_tile_scan_kernel, dim3(256, (unsigned)d), dim3(256), 0, h->stream, ntiles, info,
                           (const unsigned int*)(sc.dbase + (size_t)b * d * 256), sc.tcount);
        hipLaunchKernelGGL(rank_scatter_kernel, grid, dim3(RANK_BS), 0, h->stream, sc.buf0, sc.buf1, S, ntiles, 8 * b, info,
                           (const unsigned int*)sc.tcount);
    }
    return DEMCZ_OK;
}

// demcz_rank_normalize on a source that holds an N x d x Gcap history (a sampling handle, a derived history, a ScratchHandle)
int32_t rank_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t mode, const double* center, demcz_handle** ranked)
{
    const char* who = "demcz_rank_normalize";
    if (mode != DEMCZ_RANK_Z && mode != DEMCZ_RANK_AVERAGE)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_rank_normalize: mode is DEMCZ_RANK_Z or DEMCZ_RANK_AVERAGE");
    int32_t rc = rank_refuse_sharded(h, who);
    if (rc) return rc;
    Window win;
    rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    rc = enter_device(h);
    if (rc) return rc;
    const int64_t N = win.N, s0 = win.s0, S = win.total;
    const int d = win.d;
    if (S >= ((int64_t)1 << 31) || d > 65535)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_rank_normalize: at most 2^31 - 1 draws per parameter and 65535 parameters");
    rc = quiesce_all(h);                        // (the allocations below may synchronise the device)
    if (rc) return rc;
    std::string err;
    NewDerived dh = derived_create(h->cfg.device_id, N, d, win.w, g_from - 1, nullptr, 0, err, who);
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    RankSort rs;                                // (behind dh: the scratch goes first)
    rc = rank_sort_alloc(h, d, S, who, rs);
    if (rc) return rc;
    auto body = [&]() -> int32_t {              // (HIPCHK returns from inside: one place where every such return is settled)
        int32_t r2 = rank_sort_run(h, N, d, s0, S, center, who, rs);
        if (r2) return r2;
        const RankScratch& sc = rs.sc;
        hipLaunchKernelGGL(rank_score_kernel, dim3((unsigned)((S + RANK_BS - 1) / RANK_BS), (unsigned)d), dim3(RANK_BS), 0, h->stream,
                           (const double*)h->dchain, N, d, s0, S, rs.dcenter, (const uint64_t*)sc.buf0, (const uint64_t*)sc.buf1,
                           (const int*)(sc.info + (size_t)RANK_DIGITS * d), (const unsigned long long*)sc.nan, (int)mode, dh->dchain);
        HIPCHK(h, hipGetLastError());
        return sync_stream(h, h->stream, who);
    };
    rc = settle(body());
    if (rc) return rc;
    *ranked = dh.release();
    return DEMCZ_OK;
}

// demcz_indicator_le on such a source: a map per draw, local to the handle's own chains
int32_t indicator_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nthr, const double* thr, demcz_handle** derived)
{
    const char* who = "demcz_indicator_le";
    Window win;
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    if (nthr < 1 || nthr > 64 || (int64_t)win.d * nthr > 65535)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_indicator_le: 1 <= nthr <= 64 and d nthr <= 65535");
    rc = enter_device(h);
    if (rc) return rc;
    rc = quiesce_all(h);
    if (rc) return rc;
    const int m = win.d * nthr;
    const int64_t total = win.total * m;
    std::string err;
    NewDerived dh = derived_create(h->cfg.device_id, win.N, m, win.w, g_from - 1, thr, (int64_t)m, err, who);   // (the thresholds: its data)
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(indicator_le_kernel, dim3(blocks), dim3(256), 0, h->stream, (const double*)h->dchain, win.N, win.d, win.s0, total,
                       (int)nthr, (const double*)dh->d_design, dh->dchain);
    return finish(h, who, "indicator_le_kernel", hipGetLastError(), dh, derived);
}

int32_t rank_diagnostics_from(demcz_handle* h, int64_t g_from, int64_t g_to, double* rhat_rank, double* ess_bulk, double* ess_tail)
{
    const char* who = "demcz_rank_diagnostics";
    int32_t rc = rank_refuse_sharded(h, who);
    if (rc) return rc;
    rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    if (g_to - g_from + 1 < 4) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_rank_diagnostics: window needs at least 4 generations");
    const int d = h->cfg.d;
    const double probs[3] = {0.05, 0.5, 0.95};
    std::vector<double> q((size_t)3 * d), a((size_t)2 * d), b((size_t)d);
    rc = demcz_quantiles(h, g_from, g_to, 3, probs, q.data(), nullptr, nullptr);
    if (rc) return rc;
    if (rhat_rank || ess_bulk) {                // (each part is dropped before the next is made: it takes the same memory)
        Part zb;
        rc = rank_from(h, g_from, g_to, DEMCZ_RANK_Z, nullptr, &zb.h);
        if (!rc && ess_bulk) rc = part_rc(h, zb.h, demcz_ess(zb.h, g_from, g_to, 0, ess_bulk, nullptr, nullptr, nullptr, nullptr));
        if (!rc && rhat_rank) rc = part_rc(h, zb.h, demcz_rhat(zb.h, g_from, g_to, a.data()));
        if (rc) return rc;
    }
    if (rhat_rank) {
        Part zf;
        rc = rank_from(h, g_from, g_to, DEMCZ_RANK_Z, q.data() + d, &zf.h);             // folded at the median
        if (!rc) rc = part_rc(h, zf.h, demcz_rhat(zf.h, g_from, g_to, b.data()));
        if (rc) return rc;
        for (int p = 0; p < d; ++p)
            rhat_rank[p] = (a[p] != a[p] || b[p] != b[p]) ? std::nan("") : std::max(a[p], b[p]);
    }
    if (ess_tail) {
        std::vector<double> thr((size_t)2 * d);
        for (int p = 0; p < d; ++p) { thr[p] = q[p]; thr[(size_t)d + p] = q[(size_t)2 * d + p]; }
        Part ind;
        rc = indicator_from(h, g_from, g_to, 2, thr.data(), &ind.h);
        if (!rc) rc = part_rc(h, ind.h, demcz_ess(ind.h, g_from, g_to, 0, a.data(), nullptr, nullptr, nullptr, nullptr));
        if (rc) return rc;
        for (int p = 0; p < d; ++p) {
            const double lo = a[p], hi = a[(size_t)d + p];
            ess_tail[p] = (lo != lo || hi != hi) ? std::nan("") : std::min(lo, hi);
        }
    }
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_rank_normalize(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t mode, const double* center,
                                        demcz_handle** ranked)
{
    if (!h || !ranked) return DEMCZ_ERR_INVALID_ARGUMENT;
    *ranked = nullptr;
    DEADCHK(h);
    return rank_from(h, g_from, g_to, mode, center, ranked);
}

extern "C" int32_t demcz_rank_normalize_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t mode,
                                              const double* center, demcz_handle** ranked)
{
    if (!chain || !ranked) return DEMCZ_ERR_INVALID_ARGUMENT;
    *ranked = nullptr;
    // (the upload is freed when this call returns: only the ranked history stays)
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return rank_from(h, 1, G, mode, center, ranked); });
}

extern "C" int32_t demcz_indicator_le(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nthr, const double* thr,
                                      demcz_handle** derived)
{
    if (!h || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    if (!thr) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_indicator_le: thr is NULL");
    DEADCHK(h);
    return indicator_from(h, g_from, g_to, nthr, thr, derived);
}

extern "C" int32_t demcz_rank_diagnostics(demcz_handle* h, int64_t g_from, int64_t g_to, double* rhat_rank, double* ess_bulk,
                                          double* ess_tail)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!rhat_rank && !ess_bulk && !ess_tail) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_rank_diagnostics: every output is NULL");
    DEADCHK(h);
    return rank_diagnostics_from(h, g_from, g_to, rhat_rank, ess_bulk, ess_tail);
}

extern "C" int32_t demcz_rank_diagnostics_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G,
                                                double* rhat_rank, double* ess_bulk, double* ess_tail)
{
    if (!chain || (!rhat_rank && !ess_bulk && !ess_tail)) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr,
                       [&](demcz_handle* h) { return rank_diagnostics_from(h, 1, G, rhat_rank, ess_bulk, ess_tail); });
}

// ---- posterior densities (K13, demcz_kernels_density.h, demcz_density_host.h): histograms, pair grids, the HDI -------------------
namespace {
// The range of every parameter of a histogram: the caller's (finite, lo < hi, hi - lo finite), or with neither given the window's
// smallest and largest draw, exact, by the select at probabilities 0 and 1; where the two are equal, (x - 0.5, x + 0.5).
int32_t density_range(demcz_handle* h, int64_t g_from, int64_t g_to, const double* lo, const double* hi, const char* who,
                      std::vector<double>& rlo, std::vector<double>& rhi)
{
    const int d = h->cfg.d;
    rlo.resize((size_t)d);
    rhi.resize((size_t)d);
    if ((lo == nullptr) != (hi == nullptr)) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": give both lo and hi, or neither");
    if (lo) {
        for (int p = 0; p < d; ++p) {
            if (!(lo[p] < hi[p]) || !std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !std::isfinite(hi[p] - lo[p]))
                return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": parameter " + std::to_string(p) +
                                                           ": the range must be finite with lo < hi (and hi - lo finite)");
            rlo[p] = lo[p];
            rhi[p] = hi[p];
        }
        return DEMCZ_OK;
    }
    if (h->comm && h->nranks > 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": on a sharded handle give the range (the extremes over all ranks: "
                                                   "demcz_select_counts added on the host), then add the counts over the ranks");
    const double probs[2] = {0.0, 1.0};
    std::vector<double> q((size_t)2 * d);
    int32_t rc = demcz_quantiles(h, g_from, g_to, 2, probs, q.data(), nullptr, nullptr);
    if (rc) return rc;
    for (int p = 0; p < d; ++p) {
        double a = q[p], b = q[(size_t)d + p];
        if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(b - a))
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": parameter " + std::to_string(p) +
                                                       " has a NaN or infinite draw in the window (or extremes further apart than a "
                                                       "double holds): give a range");
        if (a == b) { a = a - 0.5; b = b + 0.5; }
        if (!(a < b))
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": parameter " + std::to_string(p) +
                                                       " is a constant too large for the range (x - 0.5, x + 0.5): give a range");
        rlo[p] = a;
        rhi[p] = b;
    }
    return DEMCZ_OK;
}

// the d edge tables of nb + 1 entries each, [p][k]
int32_t density_tables(demcz_handle* h, int nb, const std::vector<double>& lo, const std::vector<double>& hi, const char* who,
                       std::vector<double>& edges)
{
    const int d = h->cfg.d;
    edges.resize((size_t)d * (nb + 1));
    for (int p = 0; p < d; ++p)
        if (demcz_histogram_edges(nb, lo[p], hi[p], edges.data() + (size_t)p * (nb + 1)))
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": parameter " + std::to_string(p) + ": no edge table for its range");
    return DEMCZ_OK;
}

// demcz_histogram on a source that holds an N x d x Gcap history (a sampling handle, a derived history, a ScratchHandle)
int32_t histogram_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nbins, const double* lo, const double* hi, double* edges,
                       int64_t* counts, int64_t* below, int64_t* above, int64_t* nan_count)
{
    const char* who = "demcz_histogram";
    if (nbins < 1 || nbins > DENSITY_MAX_BINS)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram: 1 <= nbins <= 4096 (32-bit counters in 16 KB of LDS)");
    int32_t rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    std::vector<double> rlo, rhi, he;
    rc = density_range(h, g_from, g_to, lo, hi, who, rlo, rhi);
    if (rc) return rc;
    rc = density_tables(h, nbins, rlo, rhi, who, he);
    if (rc) return rc;
    const int d = h->cfg.d;
    const int64_t ne = (int64_t)d * (nbins + 1), nc = (int64_t)d * (nbins + 3);
    SelPlan s;
    rc = sel_prepare(h, g_from, g_to, s, ne + nc, who);
    if (rc) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(double), "scratch reuse");
    double* de = h->d_scratch + s.off;
    unsigned long long* dc = reinterpret_cast<unsigned long long*>(de + ne);
    std::vector<uint64_t> hc((size_t)nc);
    auto body = [&]() -> int32_t {
        HIPCHK(h, hipMemcpyAsync(de, he.data(), (size_t)ne * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(dc, 0, (size_t)nc * sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(histogram_kernel, dim3((unsigned)(s.cb * s.d), (unsigned)s.nchunk), dim3(DEN_BS), 0, h->stream,
                           (const double*)h->dchain, s.N, s.d, s.s0, s.w, s.cb, s.per, (int)nbins, (const double*)de, dc);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hc.data(), dc, (size_t)nc * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        return sync_stream(h, h->stream, who);
    };
    rc = body();
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }          // (copies into this call's vectors may be under way)
    for (int p = 0; p < d; ++p) {
        const uint64_t* c = hc.data() + (size_t)p * (nbins + 3);
        for (int k = 0; k < nbins; ++k) counts[(size_t)p * nbins + k] = (int64_t)c[k];
        if (below) below[p] = (int64_t)c[nbins];
        if (above) above[p] = (int64_t)c[nbins + 1];
        if (nan_count) nan_count[p] = (int64_t)c[nbins + 2];
    }
    if (edges) std::copy(he.begin(), he.end(), edges);
    return DEMCZ_OK;
}

// demcz_histogram2d on such a source
int32_t histogram2d_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t npairs, const int32_t* pairs, int32_t nbx, int32_t nby,
                         const double* lo, const double* hi, double* edges_x, double* edges_y, int64_t* counts, int64_t* outside)
{
    const char* who = "demcz_histogram2d";
    if (nbx < 1 || nby < 1 || nbx > DENSITY_MAX_SIDE || nby > DENSITY_MAX_SIDE)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: 1 <= nbx, nby <= 128 (the 32-bit counters of one pair in 64 KB of LDS)");
    if (npairs < 1) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: npairs >= 1");
    int32_t rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    const int d = h->cfg.d;
    const int64_t ncell = (int64_t)nbx * nby;
    // the distinct pairs, in order of first appearance; a repeated one is counted once and copied
    std::map<std::pair<int32_t, int32_t>, int32_t> seen;
    std::vector<int32_t> uniq, src((size_t)npairs);
    for (int i = 0; i < npairs; ++i) {
        const int32_t p = pairs[2 * i], q = pairs[2 * i + 1];
        if (p < 0 || q < 0 || p >= d || q >= d || p == q)
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: pair " + std::to_string(i) + ": need 0 <= p, q < d and p != q");
        const auto at = seen.emplace(std::make_pair(p, q), (int32_t)(uniq.size() / 2));
        if (at.second) { uniq.push_back(p); uniq.push_back(q); }
        src[i] = at.first->second;
    }
    const int64_t nu = (int64_t)uniq.size() / 2;
    if (nu * ncell > ((int64_t)1 << 27))
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: more than 2^27 cells in one call: ask for the pairs in several");
    std::vector<double> rlo, rhi, hex, hey;
    rc = density_range(h, g_from, g_to, lo, hi, who, rlo, rhi);
    if (rc) return rc;
    rc = density_tables(h, nbx, rlo, rhi, who, hex);
    if (rc) return rc;
    rc = density_tables(h, nby, rlo, rhi, who, hey);
    if (rc) return rc;
    DensityPlan plan;
    if (density_plan(d, (int32_t)nu, uniq.data(), nbx, nby, plan)) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: no plan");
    const int64_t ntiles = (int64_t)plan.tiles.size();
    static_assert(sizeof(DensityTile) % 8 == 0, "tiles lie in 8-byte words of the scratch");
    const int64_t nex = (int64_t)d * (nbx + 1), ney = (int64_t)d * (nby + 1), nc = nu * ncell,
                  nt = ntiles * (int64_t)(sizeof(DensityTile) / 8);
    SelPlan s;
    rc = sel_prepare(h, g_from, g_to, s, nex + ney + nc + nt, who);
    if (rc) return rc;
    // chunks as sel_prepare's, for ntiles x cb groups of workgroups instead of d x cb
    const int64_t groups = ntiles * s.cb;
    if (groups > 0x7fffffffll) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_histogram2d: too many tiles for one launch");
    int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>((s.w + 15) / 16, (4096 + groups - 1) / groups));
    nchunk = std::max<int64_t>(nchunk, (s.w + ((int64_t)1 << 20) - 1) >> 20);
    const int64_t per = (s.w + nchunk - 1) / nchunk;
    nchunk = (s.w + per - 1) / per;
    int most = 1;
    for (const DensityTile& T : plan.tiles) most = std::max(most, (int)T.npair);
    const size_t lds = (size_t)most * ncell * sizeof(unsigned int);       // <= cap nbx nby counters = 64 KB
    double* dex = h->d_scratch + s.off;
    double* dey = dex + nex;
    unsigned long long* dc = reinterpret_cast<unsigned long long*>(dey + ney);
    DensityTile* dt = reinterpret_cast<DensityTile*>(dc + nc);
    std::vector<uint64_t> hc((size_t)nc);
    auto body = [&]() -> int32_t {
        HIPCHK(h, hipMemcpyAsync(dex, hex.data(), (size_t)nex * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dey, hey.data(), (size_t)ney * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dt, plan.tiles.data(), (size_t)ntiles * sizeof(DensityTile), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(dc, 0, (size_t)nc * sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(histogram2d_kernel, dim3((unsigned)groups, (unsigned)nchunk), dim3(DEN_BS), lds, h->stream,
                           (const double*)h->dchain, s.N, s.d, s.s0, s.w, s.cb, per, (int)nbx, (int)nby, (const double*)dex,
                           (const double*)dey, (const DensityTile*)dt, dc);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hc.data(), dc, (size_t)nc * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        return sync_stream(h, h->stream, who);
    };
    rc = body();
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }          // (copies into this call's vectors may be under way)
    // every draw of the window is in one cell of a pair or outside it: outside = S - the cells' total
    const int64_t S = s.N * s.w;
    for (int i = 0; i < npairs; ++i) {
        const uint64_t* c = hc.data() + (size_t)src[i] * ncell;
        int64_t in = 0;
        for (int64_t k = 0; k < ncell; ++k) { counts[(size_t)i * ncell + k] = (int64_t)c[k]; in += (int64_t)c[k]; }
        if (outside) outside[i] = S - in;
    }
    if (edges_x) std::copy(hex.begin(), hex.end(), edges_x);
    if (edges_y) std::copy(hey.begin(), hey.end(), edges_y);
    return DEMCZ_OK;
}

// demcz_hdi on such a source: the ranks' sort, then the arg-min over the sorted keys
int32_t hdi_from(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nprob, const double* probs, double* hdi)
{
    const char* who = "demcz_hdi";
    if (h->comm && h->nranks > 1)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_hdi: the sort is of one handle's draws, and the interval needs those of every "
                                                   "shard: gather the window with demcz_get_history on every rank and use demcz_hdi_array "
                                                   "on the whole");
    Window win;
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    HdiSteps steps = {};
    int64_t m[DENSITY_MAX_PROBS] = {};
    if (nprob < 1 || nprob > DENSITY_MAX_PROBS || demcz_hdi_steps(win.total, nprob, probs, m))
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_hdi: 1 to 16 probabilities, each inside (0, 1)");
    for (int j = 0; j < nprob; ++j) steps.m[j] = (long long)m[j];
    rc = enter_device(h);
    if (rc) return rc;
    const int64_t N = win.N, s0 = win.s0, S = win.total;
    const int d = win.d;
    if (S >= ((int64_t)1 << 31) || d > 65535)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_hdi: at most 2^31 - 1 draws per parameter and 65535 parameters");
    rc = quiesce_all(h);                        // (the allocation below may synchronise the device)
    if (rc) return rc;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((S + 2047) / 2048, 1024));
    const size_t npart = (size_t)d * nprob * nb, nout = (size_t)d * nprob * 2;
    std::vector<double> hout(nout);
    RankSort rs;                                // (behind hout: the scratch goes first)
    rc = rank_sort_alloc(h, d, S, who, rs, npart * 16 + nout * 8);
    if (rc) return rc;
    auto body = [&]() -> int32_t {              // (HIPCHK returns from inside: one place where every such return is settled)
        int32_t r2 = rank_sort_run(h, N, d, s0, S, nullptr, who, rs);
        if (r2) return r2;
        const RankScratch& sc = rs.sc;
        static_assert(sizeof(long long) == sizeof(double), "partials");
        double* pv = static_cast<double*>(sc.extra);
        long long* pi = reinterpret_cast<long long*>(pv + npart);
        double* dout = reinterpret_cast<double*>(pi + npart);
        const int* where = sc.info + (size_t)RANK_DIGITS * d;
        hipLaunchKernelGGL(hdi_partial_kernel, dim3((unsigned)nb, (unsigned)nprob, (unsigned)d), dim3(256), 0, h->stream,
                           (const uint64_t*)sc.buf0, (const uint64_t*)sc.buf1, where, S, steps, pv, pi);
        hipLaunchKernelGGL(hdi_final_kernel, dim3((unsigned)nprob, (unsigned)d), dim3(256), 0, h->stream, (const uint64_t*)sc.buf0,
                           (const uint64_t*)sc.buf1, where, (const unsigned long long*)sc.nan, S, steps, (const double*)pv,
                           (const long long*)pi, nb, dout);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hout.data(), dout, nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return sync_stream(h, h->stream, who);
    };
    rc = settle(body());
    if (rc) return rc;
    std::copy(hout.begin(), hout.end(), hdi);
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_histogram(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nbins, const double* lo, const double* hi,
                                   double* edges, int64_t* counts, int64_t* below, int64_t* above, int64_t* nan_count)
{
    if (!h || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return histogram_from(h, g_from, g_to, nbins, lo, hi, edges, counts, below, above, nan_count);
}

extern "C" int32_t demcz_histogram_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nbins,
                                         const double* lo, const double* hi, double* edges, int64_t* counts, int64_t* below,
                                         int64_t* above, int64_t* nan_count)
{
    if (!chain || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) {
        return histogram_from(h, 1, G, nbins, lo, hi, edges, counts, below, above, nan_count);
    });
}

extern "C" int32_t demcz_histogram2d(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t npairs, const int32_t* pairs, int32_t nbx,
                                     int32_t nby, const double* lo, const double* hi, double* edges_x, double* edges_y,
                                     int64_t* counts, int64_t* outside)
{
    if (!h || !pairs || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return histogram2d_from(h, g_from, g_to, npairs, pairs, nbx, nby, lo, hi, edges_x, edges_y, counts, outside);
}

extern "C" int32_t demcz_histogram2d_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t npairs,
                                           const int32_t* pairs, int32_t nbx, int32_t nby, const double* lo, const double* hi,
                                           double* edges_x, double* edges_y, int64_t* counts, int64_t* outside)
{
    if (!chain || !pairs || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) {
        return histogram2d_from(h, 1, G, npairs, pairs, nbx, nby, lo, hi, edges_x, edges_y, counts, outside);
    });
}

extern "C" int32_t demcz_hdi(demcz_handle* h, int64_t g_from, int64_t g_to, int32_t nprob, const double* probs, double* hdi)
{
    if (!h || !probs || !hdi) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return hdi_from(h, g_from, g_to, nprob, probs, hdi);
}

extern "C" int32_t demcz_hdi_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int32_t nprob,
                                   const double* probs, double* hdi)
{
    if (!chain || !probs || !hdi) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) { return hdi_from(h, 1, G, nprob, probs, hdi); });
}

// ---- PSIS-LOO and WAIC (demcz_kernels_pointwise.h, K11 demcz_kernels_loo.h, demcz_loo_host.h) -----------------------------------
extern "C" int32_t demcz_pointwise_check(int32_t d, const char* source, const char* options)
{
    return program_compile(nullptr, demcz_prog::UNIT_POINTWISE, d, 0, source, options);
}

namespace {
// demcz_pointwise on a source that holds an N x d x Gcap history (a sampling handle, a derived history, a ScratchHandle)
int32_t pointwise_from(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t obs_from, int32_t mc, const char* source, const char* options,
                       const double* data, int64_t ndata, demcz_handle** derived)
{
    const char* who = "demcz_pointwise";
    Window win;
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    rc = data_check(h, who, data, ndata);
    if (rc) return rc;
    if (mc < 1 || mc > LOO_MAX_CHUNK || obs_from < 0)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "pointwise program: mc must be in 1.." + std::to_string(LOO_MAX_CHUNK) + " and obs_from >= 0");
    rc = enter_device(h);
    if (rc) return rc;
    demcz_prog::Module mod;
    rc = program_load(h, demcz_prog::UNIT_POINTWISE, win.d, 0, source, options, mod);
    if (rc) return rc;
    rc = quiesce_all(h);                        // (a sharded handle: the allocations below synchronise the device)
    if (rc) return rc;
    std::string err;
    NewDerived dh = derived_create(h->cfg.device_id, win.N, mc, win.w, g_from - 1, data, ndata, err, who);
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    const double* chain = h->dchain;
    const double* ddata = ndata > 0 ? dh->d_design : nullptr;
    double* out = dh->dchain;
    int mcount = mc;
    void* args[] = {&chain, &win.N, &win.s0, &win.total, &ddata, &ndata, &obs_from, &mcount, &out};
    const hipError_t e = hipModuleLaunchKernel(mod.fn[demcz_prog::POINTWISE_KERNEL], derive_blocks(win.total), 1, 1, DERIVE_THREADS, 1, 1, 0, h->stream, args, nullptr);
    return finish(h, who, "pointwise_kernel", e, dh, derived);
}

// demcz_loo_columns on such a source: the d columns of the window are the log-likelihoods of d observations
int32_t loo_columns_from(demcz_handle* h, int64_t g_from, int64_t g_to, const double* r_eff, double* elpd_loo, double* pareto_k,
                         int64_t* n_tail, double* lppd, double* p_waic)
{
    const char* who = "demcz_loo_columns";
    int32_t rc = rank_refuse_sharded(h, who);
    if (rc) return rc;
    Window win;
    rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    const int64_t N = win.N, s0 = win.s0, S = win.total;
    const int d = win.d;
    if (r_eff)
        for (int p = 0; p < d; ++p)
            if (!(r_eff[p] > 0.0) || !(r_eff[p] < INFINITY))
                return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_loo_columns: every r_eff must be in (0, inf)");
    rc = enter_device(h);
    if (rc) return rc;
    if (S >= ((int64_t)1 << 31) || d > 65535)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_loo_columns: at most 2^31 - 1 draws per column and 65535 columns");
    rc = quiesce_all(h);                        // (the allocations below may synchronise the device)
    if (rc) return rc;
    RankSort rs;
    rc = rank_sort_alloc(h, d, S, who, rs);
    if (rc) return rc;
    // [fit | part | out (4 d doubles) | n_tail (d) | r_eff (d)], every piece a multiple of 8 bytes
    const int64_t ntiles = (S + LOO_TILE - 1) / LOO_TILE;
    const size_t fit_bytes = ((size_t)d * sizeof(LooFit) + 7) / 8 * 8, npart = (size_t)d * ntiles * LOO_NPART;
    DevBlock base;                              // (behind rs: freed first)
    const hipError_t e = base.alloc(h->cfg.device_id, fit_bytes + npart * 8 + (size_t)6 * d * 8);
    if (e != hipSuccess) return fail(h, DEMCZ_ERR_HIP, std::string(who) + ": the fit table and the tile sums: " + hipGetErrorString(e));
    LooFit* fit = static_cast<LooFit*>(base.p);
    double* part = reinterpret_cast<double*>(static_cast<char*>(base.p) + fit_bytes);
    double* dout = part + npart;
    long long* dtail = reinterpret_cast<long long*>(dout + (size_t)4 * d);
    double* dreff = reinterpret_cast<double*>(dtail + d);
    std::vector<double> hout((size_t)4 * d), hreff;
    std::vector<long long> htail((size_t)d);
    auto body = [&]() -> int32_t {              // (HIPCHK returns from inside: one place where every such return is settled)
        int32_t r2 = rank_sort_run(h, N, d, s0, S, nullptr, who, rs);
        if (r2) return r2;
        const RankScratch& sc = rs.sc;
        const int* where = sc.info + (size_t)RANK_DIGITS * d;
        const double* reff = nullptr;
        if (r_eff) {
            hreff.assign(r_eff, r_eff + d);
            HIPCHK(h, hipMemcpyAsync(dreff, hreff.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, h->stream));
            reff = dreff;
        }
        hipLaunchKernelGGL(psis_fit_kernel, dim3((unsigned)d), dim3(LOO_BS), 0, h->stream, sc.buf0, sc.buf1, where,
                           (const unsigned long long*)sc.nan, reff, S, fit);
        hipLaunchKernelGGL(loo_sum_kernel, dim3((unsigned)ntiles, (unsigned)d), dim3(LOO_BS), 0, h->stream, (const uint64_t*)sc.buf0,
                           (const uint64_t*)sc.buf1, where, (const LooFit*)fit, S, ntiles, part);
        hipLaunchKernelGGL(loo_finish_kernel, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, h->stream, (const LooFit*)fit, (const double*)part,
                           S, ntiles, d, dout, dtail);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hout.data(), dout, hout.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(htail.data(), dtail, htail.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
        return sync_stream(h, h->stream, who);
    };
    rc = settle(body());
    if (rc) return rc;
    for (int p = 0; p < d; ++p) {
        if (elpd_loo) elpd_loo[p] = hout[p];
        if (pareto_k) pareto_k[p] = hout[(size_t)d + p];
        if (lppd) lppd[p] = hout[(size_t)2 * d + p];
        if (p_waic) p_waic[p] = hout[(size_t)3 * d + p];
        if (n_tail) n_tail[p] = (int64_t)htail[p];
    }
    return DEMCZ_OK;
}

// demcz_loo on such a source: chunks of observations, each evaluated, reduced and dropped
int32_t loo_from(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t nobs, const char* source, const char* options, const double* data,
                 int64_t ndata, const double* r_eff, double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic)
{
    const char* who = "demcz_loo";
    int32_t rc = rank_refuse_sharded(h, who);
    if (rc) return rc;
    rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    if (nobs < 1) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_loo: nobs must be at least 1");
    if (r_eff)
        for (int64_t i = 0; i < nobs; ++i)
            if (!(r_eff[i] > 0.0) || !(r_eff[i] < INFINITY))
                return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_loo: every r_eff must be in (0, inf)");
    const int mc = loo_chunk_width(h->cfg.N * (g_to - g_from + 1), LOO_SCRATCH_BUDGET);
    const int64_t nchunks = loo_chunk_count(nobs, mc);
    for (int64_t i = 0; i < nchunks; ++i) {
        int64_t from = 0;
        int count = 0;
        loo_chunk(nobs, mc, i, &from, &count);
        Part dh;
        rc = pointwise_from(h, g_from, g_to, from, count, source, options, data, ndata, &dh.h);
        if (rc) return rc;
        rc = part_rc(h, dh.h, loo_columns_from(dh.h, g_from, g_to, r_eff ? r_eff + from : nullptr, elpd_loo ? elpd_loo + from : nullptr,
                                                pareto_k ? pareto_k + from : nullptr, n_tail ? n_tail + from : nullptr,
                                                lppd ? lppd + from : nullptr, p_waic ? p_waic + from : nullptr));
        if (rc) return rc;
    }
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_pointwise(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t obs_from, int32_t mc, const char* source,
                                   const char* options, const double* data, int64_t ndata, demcz_handle** derived)
{
    if (!h || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    DEADCHK(h);
    return pointwise_from(h, g_from, g_to, obs_from, mc, source, options, data, ndata, derived);
}

extern "C" int32_t demcz_pointwise_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t obs_from,
                                         int32_t mc, const char* source, const char* options, const double* data, int64_t ndata,
                                         demcz_handle** derived)
{
    if (!chain || !derived) return DEMCZ_ERR_INVALID_ARGUMENT;
    *derived = nullptr;
    int32_t rc = demcz_pointwise_check(d, source, options);     // (compiled before anything is uploaded)
    if (rc) return rc;
    return with_arrays(device_id, N, d, G, chain, nullptr,
                       [&](demcz_handle* h) { return pointwise_from(h, 1, G, obs_from, mc, source, options, data, ndata, derived); });
}

extern "C" int32_t demcz_loo_columns(demcz_handle* h, int64_t g_from, int64_t g_to, const double* r_eff, double* elpd_loo,
                                     double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return loo_columns_from(h, g_from, g_to, r_eff, elpd_loo, pareto_k, n_tail, lppd, p_waic);
}

extern "C" int32_t demcz_loo_columns_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, const double* r_eff,
                                           double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic)
{
    if (!chain) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, nullptr,
                       [&](demcz_handle* h) { return loo_columns_from(h, 1, G, r_eff, elpd_loo, pareto_k, n_tail, lppd, p_waic); });
}

extern "C" int32_t demcz_loo(demcz_handle* h, int64_t g_from, int64_t g_to, int64_t nobs, const char* source, const char* options,
                             const double* data, int64_t ndata, const double* r_eff, double* elpd_loo, double* pareto_k,
                             int64_t* n_tail, double* lppd, double* p_waic)
{
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return loo_from(h, g_from, g_to, nobs, source, options, data, ndata, r_eff, elpd_loo, pareto_k, n_tail, lppd, p_waic);
}

extern "C" int32_t demcz_loo_array(int32_t device_id, const double* chain, int64_t N, int32_t d, int64_t G, int64_t nobs,
                                   const char* source, const char* options, const double* data, int64_t ndata, const double* r_eff,
                                   double* elpd_loo, double* pareto_k, int64_t* n_tail, double* lppd, double* p_waic)
{
    if (!chain) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = demcz_pointwise_check(d, source, options);     // (compiled before anything is uploaded)
    if (rc) return rc;
    return with_arrays(device_id, N, d, G, chain, nullptr, [&](demcz_handle* h) {
        return loo_from(h, 1, G, nobs, source, options, data, ndata, r_eff, elpd_loo, pareto_k, n_tail, lppd, p_waic);
    });
}

// ---- the marginal likelihood by bridge sampling (K12, demcz_kernels_bridge.h; DESIGN.md sections 3 and 4.17) ---------------------
extern "C" int32_t demcz_bridge_check(int32_t d, const char* source, const char* options)
{
    return program_compile(nullptr, demcz_prog::UNIT_BRIDGE, d, 0, source, options);
}

namespace {
// dm_log of demcz_device.h on the host: the same operations on the same bits
double bridge_dm_log_host(double x)
{
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double LG1 = 6.666666666666735130e-01, LG2 = 3.999999999940941908e-01, LG3 = 2.857142874366239149e-01,
                 LG4 = 2.222219843214978396e-01, LG5 = 1.818357216161805012e-01, LG6 = 1.531383769920937332e-01,
                 LG7 = 1.479819860511658591e-01;
    uint64_t b;
    std::memcpy(&b, &x, 8);
    uint32_t hx = (uint32_t)(b >> 32);
    const uint32_t lx = (uint32_t)b;
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    const uint64_t rb = ((uint64_t)hx << 32) | lx;
    double xr;
    std::memcpy(&xr, &rb, 8);
    const double f = xr - 1.0, hfsq = (0.5 * f) * f, s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (LG2 + w * (LG4 + w * LG6)), t2 = z * (LG1 + w * (LG3 + w * (LG5 + w * LG7)));
    const double R = t2 + t1, dk = (double)k;
    return ((((s * (hfsq + R)) + (dk * LN2_LO)) - hfsq) + f) + (dk * LN2_HI);
}

// The proposal as the kernels read it: [m | L row-major lower] (bridge_ml_words(d) doubles) and c_g.  L: d x d column-major, its
// lower triangle; a diagonal entry that is not a positive normal number is refused with the parameter's index.
int32_t bridge_pack(demcz_handle* h, int d, const double* mean, const double* L, const char* who, std::vector<double>& mL, double& cg)
{
    if (d < 1 || d > BRIDGE_MAX_D)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": d must be in 1.." + std::to_string(BRIDGE_MAX_D));
    mL.resize((size_t)bridge_ml_words(d));
    for (int p = 0; p < d; ++p) mL[p] = mean[p];
    cg = 0.0;
    for (int p = 0; p < d; ++p) {
        for (int q = 0; q <= p; ++q) mL[(size_t)d + p * (p + 1) / 2 + q] = L[(size_t)p + (size_t)d * q];
        const double lpp = L[(size_t)p + (size_t)d * p];
        if (!(lpp >= DBL_MIN) || !(lpp < INFINITY))
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": the diagonal of L must be positive and finite; it is not at parameter " +
                                                       std::to_string(p));
        cg += bridge_dm_log_host(lpp);
    }
    cg += (0.5 * (double)d) * 1.8378770664093453;        // log 2 pi
    return DEMCZ_OK;
}

// L of V = L L^T in plain double, row by row, every inner product in index order; V and L d x d column-major
int32_t bridge_cholesky(demcz_handle* h, int d, const double* V, double* L, const char* who)
{
    for (size_t i = 0; i < (size_t)d * d; ++i) L[i] = 0.0;
    for (int p = 0; p < d; ++p) {
        for (int q = 0; q < p; ++q) {
            double acc = V[(size_t)p + (size_t)d * q];
            for (int k = 0; k < q; ++k) acc = acc - L[(size_t)p + (size_t)d * k] * L[(size_t)q + (size_t)d * k];
            L[(size_t)p + (size_t)d * q] = acc / L[(size_t)q + (size_t)d * q];
        }
        double acc = V[(size_t)p + (size_t)d * p];
        for (int k = 0; k < p; ++k) acc = acc - L[(size_t)p + (size_t)d * k] * L[(size_t)p + (size_t)d * k];
        if (!(acc > 0.0) || !(acc < INFINITY))
            return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": the fit window's covariance is not positive definite: the pivot of parameter " +
                                                       std::to_string(p) + " is " + std::to_string(acc) +
                                                       " (a constant or linearly dependent parameter; a longer window or more chains)");
        L[(size_t)p + (size_t)d * p] = std::sqrt(acc);
    }
    return DEMCZ_OK;
}

// demcz_bridge_posterior on a source with a chain and a log_obj history (a sampling handle, a ScratchHandle)
int32_t bridge_posterior_from(demcz_handle* h, int64_t g_from, int64_t g_to, const double* mean, const double* L, demcz_handle** derived)
{
    const char* who = "demcz_bridge_posterior";
    Window win;
    int32_t rc = open_window(h, g_from, g_to, who, win);
    if (rc) return rc;
    if (!h->dlogobj || !h->dchain) return fail(h, DEMCZ_ERR_STATE, std::string(who) + ": the source keeps no log_obj history");
    std::vector<double> mL;
    double cg = 0.0;
    rc = bridge_pack(h, win.d, mean, L, who, mL, cg);
    if (rc) return rc;
    const void* fn = bridge_posterior_fn(win.d);
    if (!fn) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": no kernel for this d");
    rc = enter_device(h);
    if (rc) return rc;
    rc = quiesce_all(h);                        // (the allocations below may synchronise the device)
    if (rc) return rc;
    std::string err;
    // (the proposal rides in the derived history's data slot: freed with it)
    NewDerived dh = derived_create(h->cfg.device_id, win.N, 1, win.w, g_from - 1, mL.data(), (int64_t)mL.size(), err, who);
    if (!dh) return fail(h, DEMCZ_ERR_HIP, err);
    const double* chain = h->dchain;
    const double* logobj = h->dlogobj;
    const double* dmL = dh->d_design;
    double* out = dh->dchain;
    void* args[] = {&chain, &logobj, &win.N, &win.s0, &win.total, &dmL, &cg, &out};
    const hipError_t e = hipLaunchKernel(fn, dim3(derive_blocks(win.total)), dim3(DERIVE_THREADS), args, 0, h->stream);
    return finish(h, who, "bridge_posterior_kernel", e, dh, derived);
}

// What evaluates the target at the proposal's draws: a built-in target's kernel with its parameters, or a program's bridge unit
struct BridgeTarget {
    const void* fn = nullptr;                   // built-in: bridge_proposal_kernel<T, d>
    TargetParams tp{};
    hipFunction_t prog = nullptr;               // program: bridge_proposal_program_kernel
    const double* data = nullptr;               // program: device memory that outlives the call, or null: `hdata` is uploaded
    const double* hdata = nullptr;
    int64_t ndata = 0;
};

// the handle's own target
int32_t bridge_target_of(demcz_handle* h, const char* who, BridgeTarget& t)
{
    const int d = h->cfg.d;
    if (d < 1 || d > BRIDGE_MAX_D)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": d must be in 1.." + std::to_string(BRIDGE_MAX_D));
    if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM) {
        if (!h->prog_ready) return fail(h, DEMCZ_ERR_STATE, "program target: call demcz_set_program first");
        demcz_prog::Module mod;
        if (int32_t rc = program_load(h, demcz_prog::UNIT_BRIDGE, d, 0, h->prog_source.c_str(), h->prog_options.c_str(), mod)) return rc;
        t.prog = mod.fn[demcz_prog::BRIDGE_KERNEL];
        t.data = h->cfg.nobs > 0 ? h->d_design : nullptr;
        t.ndata = h->cfg.nobs;
        return DEMCZ_OK;
    }
    if (h->cfg.target_kind == DEMCZ_TARGET_HOST_CALLBACK)
        return fail(h, DEMCZ_ERR_STATE, std::string(who) + ": a host-closure handle has no target on the device: bridge sampling needs a "
                                                           "built-in or a program target");
    t.fn = bridge_proposal_fn(h->cfg.target_kind, d);
    if (!t.fn) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": no kernel for this target and d");
    t.tp = target_params(h);
    return DEMCZ_OK;
}

// a program given as text
int32_t bridge_target_program(demcz_handle* h, int d, const char* source, const char* options, const double* data, int64_t ndata,
                              const char* who, BridgeTarget& t)
{
    if (int32_t rc = data_check(h, who, data, ndata)) return rc;
    demcz_prog::Module mod;
    if (int32_t rc = program_load(h, demcz_prog::UNIT_BRIDGE, d, 0, source, options, mod)) return rc;
    t.prog = mod.fn[demcz_prog::BRIDGE_KERNEL];
    t.hdata = data;
    t.ndata = ndata;
    return DEMCZ_OK;
}

// demcz_bridge_proposal on h's device and stream: Np x wp draws of N(mean, L L^T), a2 and on request the draws
int32_t bridge_proposal_from(demcz_handle* h, int d, const BridgeTarget& t, int64_t Np, int64_t wp, uint64_t seed, const double* mean,
                             const double* L, demcz_handle** logratio, demcz_handle** draws)
{
    const char* who = "demcz_bridge_proposal";
    if (Np < 1 || wp < 1 || Np > ((int64_t)1 << 40) / wp)
        return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": need Np >= 1, wp >= 1 and at most 2^40 draws");
    std::vector<double> mL;
    double cg = 0.0;
    int32_t rc = bridge_pack(h, d, mean, L, who, mL, cg);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    rc = quiesce_all(h);                        // (the allocations below may synchronise the device)
    if (rc) return rc;
    std::string err;
    // the proposal and, behind it, a program's data ride in the a2 history's data slot
    std::vector<double> slot(mL);
    if (t.hdata && t.ndata > 0) slot.insert(slot.end(), t.hdata, t.hdata + t.ndata);
    NewDerived dx;                              // (the draws; declared first: on a failure a2 is freed before them)
    NewDerived da = derived_create(h->cfg.device_id, Np, 1, wp, 0, slot.data(), (int64_t)slot.size(), err, who);
    if (!da) return fail(h, DEMCZ_ERR_HIP, err);
    if (draws) {
        dx = derived_create(h->cfg.device_id, Np, d, wp, 0, nullptr, 0, err, who);
        if (!dx) return fail(h, DEMCZ_ERR_HIP, err);
    }
    int64_t N = Np, total = Np * wp, ndata = t.ndata;
    const double* dmL = da->d_design;
    const double* ddata = t.data ? t.data : (t.hdata && t.ndata > 0) ? da->d_design + mL.size() : nullptr;
    double* a2 = da->dchain;
    double* xs = dx ? dx->dchain : nullptr;
    hipError_t e;
    if (t.prog) {
        void* args[] = {&N, &total, &seed, &dmL, &cg, &ddata, &ndata, &a2, &xs};
        e = hipModuleLaunchKernel(t.prog, derive_blocks(total), 1, 1, DERIVE_THREADS, 1, 1, 0, h->stream, args, nullptr);
    } else {
        TargetParams tp = t.tp;
        void* args[] = {&tp, &N, &total, &seed, &dmL, &cg, &a2, &xs};
        e = hipLaunchKernel(t.fn, dim3(derive_blocks(total)), dim3(DERIVE_THREADS), args, 0, h->stream);
    }
    rc = finish(h, who, "bridge_proposal_kernel", e, da, logratio);
    if (!rc && draws) *draws = dx.release();
    return rc;
}

// updates queued between two synchronisations (DEMCZ_BRIDGE_BATCH: 1..64; the result does not depend on it)
int bridge_batch()
{
    if (const char* s = getenv("DEMCZ_BRIDGE_BATCH"); s && *s) {
        const long v = strtol(s, nullptr, 10);
        if (v >= 1 && v <= 64) return (int)v;
    }
    return 4;
}

struct BridgeResult {
    double logml = NAN, moments[4] = {NAN, NAN, NAN, NAN};
    int64_t iterations = 0, n_nan = 0;
    int32_t converged = 0;
};

int32_t bridge_iterate_from(demcz_handle* post, int64_t g_from, int64_t g_to, demcz_handle* prop, int64_t gp_from, int64_t gp_to, double neff,
                            double tol, int64_t max_iter, BridgeResult& res, demcz_handle** f2)
{
    const char* who = "demcz_bridge_iterate";
    int32_t rc = check_hist_range(post, g_from, g_to, who);
    if (rc) return rc;
    rc = part_rc(post, prop, check_hist_range(prop, gp_from, gp_to, who));       // (post is the handle the caller asks about)
    if (rc) return rc;
    if (post->cfg.d != 1 || prop->cfg.d != 1 || !post->dchain || !prop->dchain)
        return fail(post, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": both histories must have one column");
    if (post->cfg.device_id != prop->cfg.device_id)
        return fail(post, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": the two histories must be on one device");
    if ((post->comm && post->nranks > 1) || (prop->comm && prop->nranks > 1)) return rank_refuse_sharded(post->comm ? post : prop, who);
    if (!(tol >= 0.0) || max_iter < 1 || neff != neff)
        return fail(post, DEMCZ_ERR_INVALID_ARGUMENT, std::string(who) + ": need tol >= 0, max_iter >= 1 and neff a number");
    int64_t n1 = post->cfg.N * (g_to - g_from + 1), n2 = prop->cfg.N * (gp_to - gp_from + 1);
    HIPCHK(post, hipSetDevice(post->cfg.device_id));
    rc = live_verify(post);
    if (rc) return rc;
    rc = part_rc(post, prop, live_verify(prop));
    if (rc) return rc;
    rc = quiesce_all(post);
    if (rc) return rc;
    rc = part_rc(post, prop, sync_stream(prop, prop->stream, who));      // (what wrote a2 ran on its own stream)
    if (rc) return rc;
    const double ne = (neff > 0.0) ? neff : (double)n1;
    double s1 = ne / (ne + (double)n2), s2 = 1.0 - s1;
    const double* a1 = post->dchain + post->cfg.N * (g_from - post->g0 - 1);
    const double* a2 = prop->dchain + prop->cfg.N * (gp_from - prop->g0 - 1);
    int64_t ntiles = (std::max(n1, n2) + BRIDGE_TILE - 1) / BRIDGE_TILE;
    std::string err;
    NewDerived df;
    if (f2) {
        df = derived_create(post->cfg.device_id, post->cfg.N, 1, g_to - g_from + 1, g_from - 1, nullptr, 0, err, who);
        if (!df) return fail(post, DEMCZ_ERR_HIP, err);
    }
    // [state | part (2 ntiles BRIDGE_NPART doubles)]
    const size_t st_bytes = (sizeof(BridgeState) + 7) / 8 * 8;
    DevBlock base;                              // (behind df: freed first)
    const hipError_t e = base.alloc(post->cfg.device_id, st_bytes + (size_t)2 * ntiles * BRIDGE_NPART * 8);
    if (e != hipSuccess) return fail(post, DEMCZ_ERR_HIP, std::string(who) + ": the tile sums: " + hipGetErrorString(e));
    BridgeState* st = static_cast<BridgeState*>(base.p);
    double* part = reinterpret_cast<double*>(static_cast<char*>(base.p) + st_bytes);
    double* f2out = df ? df->dchain : nullptr;
    BridgeState hs;
    const int batch = bridge_batch();
    hipStream_t s = post->stream;
    auto body = [&]() -> int32_t {              // (HIPCHK returns from inside: one place where every such return is settled)
        HIPCHK(post, hipMemsetAsync(st, 0, st_bytes, s));
        int64_t tiles1 = (n1 + BRIDGE_TILE - 1) / BRIDGE_TILE;               // (<= ntiles: the maxima fit in part)
        for (int stage = 0; stage < 2; ++stage) {
            void* args[] = {&a1, &n1, &tiles1, &stage, &part, &st};
            HIPCHK(post, hipLaunchKernel(bridge_rho0_fn(), dim3(stage ? 1u : (unsigned)tiles1), dim3(BRIDGE_BS), args, 0, s));
        }
        long long mi = (long long)max_iter;
        auto round = [&](int final) -> hipError_t {
            double* fo = final ? f2out : nullptr;
            void* sa[] = {&a2, &n2, &a1, &n1, &s1, &s2, &final, &st, &part, &fo};
            hipError_t e2 = hipLaunchKernel(bridge_sum_fn(), dim3((unsigned)ntiles, 2), dim3(BRIDGE_BS), sa, 0, s);
            if (e2 != hipSuccess) return e2;
            void* fa[] = {&part, &ntiles, &n2, &n1, &tol, &mi, &final, &st};
            return hipLaunchKernel(bridge_finish_fn(), dim3(1), dim3(64), fa, 0, s);
        };
        for (int64_t queued = 0;;) {
            for (int b = 0; b < batch && queued < max_iter; ++b, ++queued) HIPCHK(post, round(0));
            HIPCHK(post, hipMemcpyAsync(&hs, st, sizeof(BridgeState), hipMemcpyDeviceToHost, s));
            int32_t r2 = sync_stream(post, s, who);
            if (r2) return r2;
            if (hs.done || queued >= max_iter) break;
        }
        HIPCHK(post, round(1));
        HIPCHK(post, hipMemcpyAsync(&hs, st, sizeof(BridgeState), hipMemcpyDeviceToHost, s));
        return sync_stream(post, s, who);
    };
    rc = settle(body());
    if (rc) return rc;
    res.logml = hs.rho;
    res.iterations = (int64_t)hs.iterations;
    res.converged = hs.converged;
    res.n_nan = (int64_t)hs.n_nan;
    const bool ok = hs.rho == hs.rho;
    res.moments[0] = ok ? hs.mean[0] : NAN;
    res.moments[1] = ok ? hs.var[0] : NAN;
    res.moments[2] = ok ? hs.mean[1] : NAN;
    res.moments[3] = ok ? hs.var[1] : NAN;
    if (f2) *f2 = df.release();
    return DEMCZ_OK;
}

struct BridgeOut {
    double *logml, *se_logml;
    int64_t* iterations;
    int32_t* converged;
    int64_t *n_post, *n_prop;
    double* neff;
    int64_t* n_nan;
    double *ess_f2, *mean, *L;
};

// the whole pipeline on a source with chain and log_obj; `t` evaluates the target
int32_t bridge_from(demcz_handle* h, const BridgeTarget& t, int64_t g_from, int64_t g_to, uint64_t seed, double neff, double tol,
                    int64_t max_iter, const BridgeOut& o)
{
    const char* who = "demcz_bridge";
    int32_t rc = rank_refuse_sharded(h, who);
    if (rc) return rc;
    rc = check_hist_range(h, g_from, g_to, who);
    if (rc) return rc;
    const int64_t w = g_to - g_from + 1, hw = w / 2, N = h->cfg.N;
    if (w < 4) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_bridge: window needs at least 4 generations");
    const int d = h->cfg.d;
    if (d > BRIDGE_MAX_D) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_bridge: d must be in 1.." + std::to_string(BRIDGE_MAX_D));
    std::vector<double> m((size_t)d), V((size_t)d * d), L((size_t)d * d);
    rc = demcz_mean_cov(h, g_from, g_from + hw - 1, m.data(), V.data());
    if (rc) return rc;
    rc = bridge_cholesky(h, d, V.data(), L.data(), who);
    if (rc) return rc;
    Part post, prop, f2;                        // (dropped when this call returns: f2, prop, post)
    BridgeResult res;
    double ess = NAN;
    rc = bridge_posterior_from(h, g_from + hw, g_to, m.data(), L.data(), &post.h);
    if (!rc) rc = bridge_proposal_from(h, d, t, N, w - hw, seed, m.data(), L.data(), &prop.h, nullptr);
    if (!rc) rc = bridge_iterate_from(post.h, g_from + hw, g_to, prop.h, 1, w - hw, neff, tol, max_iter, res, &f2.h);
    // (not part_rc: the two producers report on h, only bridge_iterate_from on post, and its message moves up where h has none)
    if (rc && post.h && !post.h->err.empty() && h->err.empty()) h->err = post.h->err;
    if (!rc && res.logml == res.logml && w - hw >= 4) {
        int32_t conv = 0;
        rc = part_rc(h, f2.h, demcz_ess(f2.h, g_from + hw, g_to, 0, &ess, nullptr, nullptr, nullptr, &conv));
    }
    if (rc) return rc;
    const int64_t n1 = N * (w - hw), n2 = n1;
    double se = NAN;
    if (res.logml == res.logml) {
        const double re2 = res.moments[1] / ((double)n2 * (res.moments[0] * res.moments[0])) +
                           res.moments[3] / (ess * (res.moments[2] * res.moments[2]));
        se = std::sqrt(re2);
    }
    if (o.logml) *o.logml = res.logml;
    if (o.se_logml) *o.se_logml = se;
    if (o.iterations) *o.iterations = res.iterations;
    if (o.converged) *o.converged = res.converged;
    if (o.n_post) *o.n_post = n1;
    if (o.n_prop) *o.n_prop = n2;
    if (o.neff) *o.neff = (neff > 0.0) ? neff : (double)n1;
    if (o.n_nan) *o.n_nan = res.n_nan;
    if (o.ess_f2) *o.ess_f2 = ess;
    if (o.mean) std::copy(m.begin(), m.end(), o.mean);
    if (o.L) std::copy(L.begin(), L.end(), o.L);
    return DEMCZ_OK;
}
}  // namespace

extern "C" int32_t demcz_bridge_posterior(demcz_handle* h, int64_t g_from, int64_t g_to, const double* mean, const double* L,
                                          demcz_handle** derived)
{
    if (derived) *derived = nullptr;
    NOT_DERIVED(h);
    if (!h || !derived || !mean || !L) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    return bridge_posterior_from(h, g_from, g_to, mean, L, derived);
}

extern "C" int32_t demcz_bridge_posterior_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d,
                                                int64_t G, const double* mean, const double* L, demcz_handle** derived)
{
    if (derived) *derived = nullptr;
    if (!chain || !log_obj || !derived || !mean || !L) return DEMCZ_ERR_INVALID_ARGUMENT;
    return with_arrays(device_id, N, d, G, chain, log_obj, [&](demcz_handle* h) { return bridge_posterior_from(h, 1, G, mean, L, derived); });
}

extern "C" int32_t demcz_bridge_proposal(demcz_handle* h, int64_t Np, int64_t wp, uint64_t seed, const double* mean, const double* L,
                                         demcz_handle** logratio, demcz_handle** draws)
{
    if (logratio) *logratio = nullptr;
    if (draws) *draws = nullptr;
    NOT_DERIVED(h);
    if (!h || !logratio || !mean || !L) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    BridgeTarget t;
    int32_t rc = bridge_target_of(h, "demcz_bridge_proposal", t);
    if (rc) return rc;
    return bridge_proposal_from(h, h->cfg.d, t, Np, wp, seed, mean, L, logratio, draws);
}

extern "C" int32_t demcz_bridge_proposal_program(int32_t device_id, int32_t d, int64_t Np, int64_t wp, uint64_t seed, const double* mean,
                                                 const double* L, const char* source, const char* options, const double* data,
                                                 int64_t ndata, demcz_handle** logratio, demcz_handle** draws)
{
    if (logratio) *logratio = nullptr;
    if (draws) *draws = nullptr;
    if (!logratio || !mean || !L) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = demcz_bridge_check(d, source, options);        // (compiled before a device is touched)
    if (rc) return rc;
    // (no arrays: a 1 x d x 1 handle that only names the device and brings a stream)
    return with_arrays(device_id, 1, d, 1, nullptr, nullptr, [&](demcz_handle* h) {
        BridgeTarget t;
        int32_t r2 = bridge_target_program(h, d, source, options, data, ndata, "demcz_bridge_proposal_program", t);
        return r2 ? r2 : bridge_proposal_from(h, d, t, Np, wp, seed, mean, L, logratio, draws);
    });
}

extern "C" int32_t demcz_bridge_iterate(demcz_handle* post, int64_t g_from, int64_t g_to, demcz_handle* prop, int64_t gp_from,
                                        int64_t gp_to, double neff, double tol, int64_t max_iter, double* logml, int64_t* iterations,
                                        int32_t* converged, double* moments, int64_t* n_nan, demcz_handle** f2)
{
    if (f2) *f2 = nullptr;
    if (!post || !prop) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(post);
    DEADCHK(prop);
    BridgeResult res;
    int32_t rc = bridge_iterate_from(post, g_from, g_to, prop, gp_from, gp_to, neff, tol, max_iter, res, f2);
    if (rc) return rc;
    if (logml) *logml = res.logml;
    if (iterations) *iterations = res.iterations;
    if (converged) *converged = res.converged;
    if (moments) std::copy(res.moments, res.moments + 4, moments);
    if (n_nan) *n_nan = res.n_nan;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_bridge(demcz_handle* h, int64_t g_from, int64_t g_to, uint64_t seed, double neff, double tol, int64_t max_iter,
                                double* logml, double* se_logml, int64_t* iterations, int32_t* converged, int64_t* n_post,
                                int64_t* n_prop, double* neff_used, int64_t* n_nan, double* ess_f2, double* mean_out, double* L_out)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    int32_t rc = rank_refuse_sharded(h, "demcz_bridge");
    if (rc) return rc;
    BridgeTarget t;
    rc = bridge_target_of(h, "demcz_bridge", t);
    if (rc) return rc;
    const BridgeOut o{logml, se_logml, iterations, converged, n_post, n_prop, neff_used, n_nan, ess_f2, mean_out, L_out};
    return bridge_from(h, t, g_from, g_to, seed, neff, tol, max_iter, o);
}

extern "C" int32_t demcz_bridge_array(int32_t device_id, const double* chain, const double* log_obj, int64_t N, int32_t d, int64_t G,
                                      const char* source, const char* options, const double* data, int64_t ndata, uint64_t seed,
                                      double neff, double tol, int64_t max_iter, double* logml, double* se_logml, int64_t* iterations,
                                      int32_t* converged, int64_t* n_post, int64_t* n_prop, double* neff_used, int64_t* n_nan,
                                      double* ess_f2, double* mean_out, double* L_out)
{
    if (!chain || !log_obj) return DEMCZ_ERR_INVALID_ARGUMENT;
    int32_t rc = demcz_bridge_check(d, source, options);        // (compiled before anything is uploaded)
    if (rc) return rc;
    const BridgeOut o{logml, se_logml, iterations, converged, n_post, n_prop, neff_used, n_nan, ess_f2, mean_out, L_out};
    return with_arrays(device_id, N, d, G, chain, log_obj, [&](demcz_handle* h) {
        BridgeTarget t;
        int32_t r2 = bridge_target_program(h, d, source, options, data, ndata, "demcz_bridge_array", t);
        return r2 ? r2 : bridge_from(h, t, 1, G, seed, neff, tol, max_iter, o);
    });
}

extern "C" int32_t demcz_get_info(const demcz_handle* h, int64_t* M, int64_t* launches_window, int32_t* lanes_per_chain)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (M) *M = h->M_app;
    if (launches_window) *launches_window = h->launches;
    if (lanes_per_chain) *lanes_per_chain = h->prog_wave ? DEMCZ_LAYOUT_PROGRAM_WAVE : (h->split_kind == SPLIT_WAVE) ? DEMCZ_LAYOUT_SPLIT_WAVE : h->lanes;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_selftest_draws(int32_t device_id, uint64_t seed, uint64_t chain, uint64_t blk0, int32_t n,
                                        uint64_t* words, double* normals, double* logu)
{
    if (n < 1 || !words || !normals || !logu) return DEMCZ_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, DEMCZ_ERR_NO_DEVICE, "demcz_selftest_draws: no HIP device visible");
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, DEMCZ_ERR_HIP, "hipSetDevice failed");
    uint64_t* dw = nullptr; double* dn = nullptr; double* dl = nullptr;
    int32_t rc = DEMCZ_OK;
    if (hipMalloc((void**)&dw, (size_t)n * 16) != hipSuccess || hipMalloc((void**)&dn, (size_t)n * 16) != hipSuccess ||
        hipMalloc((void**)&dl, (size_t)n * 8) != hipSuccess) {
        rc = fail(nullptr, DEMCZ_ERR_HIP, "demcz_selftest_draws: hipMalloc failed");
    } else {
        hipLaunchKernelGGL(selftest_draws_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, seed, chain, blk0, (int)n, dw, dn, dl);
        if (hipMemcpy(words, dw, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(normals, dn, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(logu, dl, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(nullptr, DEMCZ_ERR_HIP, "demcz_selftest_draws: kernel or copy failed");
    }
    if (dw) (void)hipFree(dw);
    if (dn) (void)hipFree(dn);
    if (dl) (void)hipFree(dl);
    return rc;
}

#ifdef DEMCZ_STAMPS
// Diagnostic build only: the stamps of the last split-layout launch (16 per workgroup, first `n_wg` workgroups).
extern "C" int32_t demcz_debug_read_stamps(demcz_handle* h, unsigned long long* out, int64_t n_wg)
{
    NOT_DERIVED(h);
    if (!h || !out || n_wg < 0 || n_wg > DEMCZ_STAMP_WGS || !h->d_stamps) return DEMCZ_ERR_INVALID_ARGUMENT;
    SYNCCHK(h, h->stream);
    HIPCHK(h, hipMemcpy(out, h->d_stamps, (size_t)n_wg * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return DEMCZ_OK;
}
#endif

static int32_t run_checked_body(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature,
                                int64_t every, double threshold, int64_t* g_stop, int32_t* n_checks,
                                double* rhat_max, int32_t n_max, double* rhat_last)
{
    const int d = h->cfg.d;
    int32_t checks = 0;
    int64_t g = g_from;
    if (g_stop) *g_stop = g_to;
    // threshold <= 0: nothing is decided on the statistic, so the checks are only enqueued between the slabs
    // (results land in pinned host memory) and read once at the end: the GPU never waits for the host.
    const bool monitor = !(threshold > 0.0);
    const int64_t max_checks = (g_to - g_from + 1) / every + 2;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (max_checks * d > h->pinned_cap) {
        { int32_t rcq = quiesce_all(h); if (rcq) return rcq; }
        SYNCCHK(h, h->stream);
        if (h->pinned_rhat) (void)host_free(h->pinned_rhat);
        h->pinned_rhat = nullptr; h->pinned_cap = 0;
        const int64_t cap = std::max<int64_t>(max_checks, 1024) * d;       // (no reallocation between calls of different length)
        HIPCHK(h, host_malloc((void**)&h->pinned_rhat, (size_t)cap * sizeof(double)));
        h->pinned_cap = cap;
    }
    double* pinned = h->pinned_rhat;
    auto max_of = [d](const double* r) {
        double mx = r[0];
        for (int p = 1; p < d; ++p) mx = (r[p] > mx || r[p] != r[p]) ? r[p] : mx;      // a NaN stays
        return mx;
    };
    int32_t rc = DEMCZ_OK;
    // With a threshold the decision needs the statistic on the host.  Where the run can be rolled back cheaply (one GPU,
    // immediate visibility, appends owned by the library, no temperature upload per slab) the next slab is enqueued
    // BEFORE waiting for it, so the GPU does not idle over the host's round trip; a stop then discards that slab:
    // X, log_obj and the archive size go back to what they were, the rows it appended become unwritten again.
    const bool speculate = !monitor && !h->comm && h->lag == 0 && !h->external_append && !temperature;
    const int64_t N = h->cfg.N;
    if (speculate) {
        if (!h->d_spec_X) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_spec_X, (size_t)N * d * sizeof(double)));
        if (!h->d_spec_lp) HIPCHK(h, dev_malloc(h->cfg.device_id, (void**)&h->d_spec_lp, (size_t)N * sizeof(double)));
        if (!h->spec_ev) HIPCHK(h, hipEventCreateWithFlags(&h->spec_ev, hipEventDisableTiming));
    }
    bool ahead = false;                 // the slab starting at g has already been enqueued
    // Nothing decided per slab, one GPU, immediate visibility, appends owned by the library: consecutive slabs are ONE demcz_run
    // call -- as few window launches as the record span allows, no launch boundary, event bracket or stream hop per slab -- and
    // their checks one batch on the side stream, gated on the call's last launch, beside the next group (slab_group_end,
    // demcz_slab_plan.h; the call's last slab stays a launch of its own, so that one slab's check trails the call as before).
    const bool grouped = monitor && !h->comm && h->lag == 0 && !h->external_append;
    int64_t max_slabs = 1;
    if (grouped && h->cfg.Gcap > 0) {
        // the largest batch's scratch, before anything is enqueued (growing it synchronises): at most 256 MiB of slices, and
        // what the span allows whatever the length of THIS call -- a longer call later finds it there
        const int64_t need1 = rhat_need(N * d, d, rhat_chunks(every / 2));
        const int64_t ls0 = live_span(h);
        max_slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(SLAB_GROUP_MAX, ((int64_t)1 << 25) / need1), (ls0 > 0 ? ls0 : h->cfg.Gcap) / every + 1));
        rc = ensure_scratch(h, max_slabs * (need1 + d));
    }
    // where a launch has to start: at the debug hook's generation; where a redo goes LIVE again (demcz_run re-arms at its entry)
    auto cut_now = [h]() {
        int64_t cut = 0;
        if (h->live_fault_polls != 0) cut = h->live_fault_g;
        if (h->no_live && h->rearm_from >= 0 && (cut == 0 || h->rearm_from + 1 < cut)) cut = h->rearm_from + 1;
        return cut;
    };
    while (g <= g_to && rc == DEMCZ_OK) {
        int64_t nxt = std::min(g_to, slab_end_at_or_after(g, every));
        RunHints hints;
        if (grouped) {
            const int64_t ls = live_span(h);
            const int64_t span = ls > 0 ? ls : INT64_MAX;
            nxt = slab_group_end(g, g_to, every, span, cut_now(), max_slabs);
            hints.bracket_slabs = (int32_t)(slab_ends_in(g, nxt, every) + (nxt % every != 0 ? 1 : 0));
            // (what the call's last launch prepares draws for: the first launch of the next group)
            hints.next_ngen = nxt < g_to ? std::min<int64_t>(span, slab_group_end(nxt + 1, g_to, every, span, cut_now(), max_slabs) - nxt) : 0;
        }
        if (!ahead) rc = run_call(h, g, nxt, gamma, temperature ? temperature + (g - g_from) : nullptr, hints);
        ahead = false;
        if (rc) break;
        // the checks of the slab ends inside g..nxt (demcz.jl:39-41): windows c0 - every + 1 .. c0, c0 + 1 .. c0 + every, ...
        int64_t c0 = slab_end_at_or_after(g, every);
        while (c0 <= nxt && c0 - every < h->g0) c0 += every;
        const int64_t nck = c0 <= nxt ? (nxt - c0) / every + 1 : 0;
        if (nck > 0) {
            double* slot = pinned + (size_t)checks * d;
            // (the call's last slab: nothing follows it on the compute stream, so its check goes there -- no hop to the side
            //  stream, ~10 us of event latency, at the end of every call)
            rc = rhat_enqueue(h, c0 - every + 1, c0, slot, /*side=*/monitor && nxt < g_to, (int)nck);
            if (rc) break;
            checks += (int32_t)nck;
            if (!monitor) {
                int64_t M_before = 0;
                if (speculate && nxt < g_to) {
                    if (hipEventRecord(h->spec_ev, h->stream) != hipSuccess) { rc = fail(h, DEMCZ_ERR_HIP, "demcz_run_checked: event failed"); break; }
                    if (hipMemcpyAsync(h->d_spec_X, h->dX, (size_t)N * d * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
                        hipMemcpyAsync(h->d_spec_lp, h->dlp, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
                        rc = fail(h, DEMCZ_ERR_HIP, "demcz_run_checked: snapshot failed");
                        break;
                    }
                    M_before = h->M_app;
                    const int64_t nn = std::min(g_to, slab_end_at_or_after(nxt + 1, every));
                    rc = demcz_run(h, nxt + 1, nn, gamma, nullptr);
                    if (rc) break;
                    ahead = true;
                    if ((rc = sync_event(h, h->spec_ev, "demcz_run_checked")) != DEMCZ_OK) break;
                } else if ((rc = sync_stream(h, h->stream, "demcz_run_checked")) != DEMCZ_OK) {
                    break;
                }
                if (max_of(slot) < threshold) {                  // demcz.jl:43
                    if (g_stop) *g_stop = nxt;
                    if (ahead) {        // discard the slab that ran ahead
                        if ((rc = sync_stream(h, h->stream, "demcz_run_checked")) != DEMCZ_OK) break;
                        rc = check_live_err(h);
                        if (rc) break;
                        if (hipMemcpyAsync(h->dX, h->d_spec_X, (size_t)N * d * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
                            hipMemcpyAsync(h->dlp, h->d_spec_lp, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
                            rc = fail(h, DEMCZ_ERR_HIP, "demcz_run_checked: restore failed");
                            break;
                        }
                        const size_t rest = (size_t)(h->M_app - M_before) * (size_t)h->ZS;
                        if (rest > 0) {
                            hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, h->stream,
                                               reinterpret_cast<unsigned long long*>(h->dZ + (size_t)M_before * h->ZS), rest, LIVE_SENTINEL);
                            if (hipGetLastError() != hipSuccess) { rc = fail(h, DEMCZ_ERR_HIP, "demcz_run_checked: restore failed"); break; }
                        }
                        // its history slots read as never written again (zeros, demcz.jl:24)
                        const int64_t s_lo = nxt - h->g0, s_hi = std::min<int64_t>(h->g_done - h->g0, h->cfg.Gcap);
                        if (s_hi > s_lo &&
                            (hipMemsetAsync(h->dchain + (size_t)N * d * s_lo, 0, (size_t)N * d * (s_hi - s_lo) * sizeof(double), h->stream) != hipSuccess ||
                             hipMemsetAsync(h->dlogobj + (size_t)N * s_lo, 0, (size_t)N * (s_hi - s_lo) * sizeof(double), h->stream) != hipSuccess)) {
                            rc = fail(h, DEMCZ_ERR_HIP, "demcz_run_checked: restore failed");
                            break;
                        }
                        if (h->hs_on) { h->after_launch_ev = nullptr; rc = stream_history(h, nxt + 1, h->g_done); if (rc) break; }   // (the mirrors read zeros there too)
                        h->M_app = M_before;
                        h->M = M_before;
                        h->g_done = nxt;
                        if ((rc = rec_scrub(h)) != DEMCZ_OK) break;
                        if (!h->live_log.empty() && h->live_log.back().g_from == nxt + 1) h->live_log.pop_back();     // the discarded slab is not to be redone
                        while (!h->acc_log.empty() && h->acc_log.back().g_last > nxt) h->acc_log.pop_back();
                    }
                    break;
                }
            }
        }
        g = nxt + 1;
    }
    // the verdict on the call's row hand-offs (demcz_run_checked, below) needs the error word on the host: its copy goes behind
    // the last launch NOW, so that it travels while the last slab's statistic is still being made -- not as a blocking copy of
    // its own after everything else (one host round trip less at the end of every call: ~30 us)
    h->pinned_err_launches = -1;
    if (rc == DEMCZ_OK && !h->live_log.empty() && h->peer_mode != 2) {
        if (!h->pinned_err && host_malloc((void**)&h->pinned_err, 4 * sizeof(unsigned int)) != hipSuccess) { h->pinned_err = nullptr; (void)hipGetLastError(); }
        if (h->pinned_err && hipMemcpyAsync(h->pinned_err, h->d_live_err, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream) == hipSuccess)
            h->pinned_err_launches = h->launches;
    }
    if (rc == DEMCZ_OK) rc = sync_stream(h, h->stream, "demcz_run_checked");
    if (rc == DEMCZ_OK && h->diag_stream) rc = sync_stream(h, h->diag_stream, "demcz_run_checked");
    if (rc == DEMCZ_OK && h->prod_stream) rc = sync_stream(h, h->prod_stream, "demcz_run_checked");
    if (rc == DEMCZ_OK && h->comm_stream) rc = sync_stream(h, h->comm_stream, "demcz_run_checked");
    if (rc == DEMCZ_OK) {
        for (int32_t i = 0; i < checks; ++i)
            if (rhat_max && i < n_max) rhat_max[i] = max_of(pinned + (size_t)i * d);
        if (rhat_last && checks > 0) std::copy(pinned + (size_t)(checks - 1) * d, pinned + (size_t)checks * d, rhat_last);
        if (n_checks) *n_checks = checks;
    }
    return rc;
}

extern "C" int32_t demcz_run_checked(demcz_handle* h, int64_t g_from, int64_t g_to, double gamma, const double* temperature,
                                     int64_t every, double threshold, int64_t* g_stop, int32_t* n_checks,
                                     double* rhat_max, int32_t n_max, double* rhat_last)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    DEADCHK(h);
    if (every < 4 || g_from < 1 || g_to < g_from) return fail(h, DEMCZ_ERR_INVALID_ARGUMENT, "demcz_run_checked: need every >= 4 and 1 <= g_from <= g_to");
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_run_checked: call demcz_set_state first");
    if (h->peer_mode == 1 || h->peer_mode == 3) return fail(h, DEMCZ_ERR_STATE, "demcz_run_checked: replica groups and host-mediated peers are driven call by call (demcz_run, demcz_rhat_partial)");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    // everything before this call is verified first, so that a failed LIVE hand-off inside it rolls back to HERE
    int32_t rc = live_verify(h);
    if (rc) return rc;
    // (a handle waiting to go LIVE again does so at this call's first slab or -- in a redo -- at a later one, never at a point of
    //  a fresh call that is not its entry: the snapshot a failure goes back to must be the entry's)
    if (h->no_live && h->rearm_from >= g_from) h->rearm_from = g_from - 1;
    const bool pacing = (getenv("DEMCZ_NO_HOST_PACING") == nullptr);
    for (;;) {
        h->host_paced = pacing;
        h->in_checked = true;
        rc = run_checked_body(h, g_from, g_to, gamma, temperature, every, threshold, g_stop, n_checks, rhat_max, n_max, rhat_last);
        h->host_paced = false;
        h->in_checked = false;
        if (h->live_log.empty()) break;
        // the statistics and the stop decision above may rest on a slab whose row hand-off failed: look, and if so undo the whole
        // call and make it again -- one launch per K-window up to the slab that holds the generation whose row never came, LIVE
        // again behind it while the handle has re-arms left (live_rollback), every slab of the redo logged against THIS call's
        // entry (`replaying`).  A redo that fails too is redone the same way; without a re-arm left it cannot fail.
        // (a run that failed for another reason on THIS rank only must not leave the others waiting in the reduction below: the
        //  communicator's deadline covers it)
        if (rc != DEMCZ_OK && h->peer_mode == 2) break;
        bool failed = false;
        { int32_t rcf = live_failed(h, failed); if (rcf) { rc = rcf; break; } }
        if (!failed) { h->live_log.clear(); break; }
        std::vector<demcz_handle::RunCall> dropped;
        rc = live_rollback(h, dropped);
        if (rc) break;
        h->replaying = true;
    }
    h->replaying = false;
    return rc;
}

// ---- diagnostic entry points (not part of the contract of SURVEY.md 8(b); benchmarks and tests only) ----------
extern "C" int32_t demcz_set_live_spin_limit(demcz_handle* h, int32_t polls)
{
    NOT_DERIVED(h);
    if (!h || polls < 0) return DEMCZ_ERR_INVALID_ARGUMENT;
    h->live_spin_limit = (unsigned int)polls;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_live_rearms(demcz_handle* h, int32_t n)
{
    NOT_DERIVED(h);
    if (!h || n < 0) return DEMCZ_ERR_INVALID_ARGUMENT;
    h->live_rearms_left = n;
    if (h->peer_mode == 1 && h->group) {
        h->group->rearms_left = n;
        for (demcz_handle* m : h->group->members) m->live_rearms_left = n;
    }
    if (n == 0) h->rearm_from = -1;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_live_rearms(const demcz_handle* h, int32_t* rearms, int32_t* left)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (rearms) *rearms = h->live_rearms;
    if (left) *left = h->live_rearms_left;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_debug_set_live_fault(demcz_handle* h, int32_t polls, int64_t g_from)
{
    NOT_DERIVED(h);
    if (!h || polls < -1 || g_from < 0) return DEMCZ_ERR_INVALID_ARGUMENT;
    h->live_fault_polls = polls;
    h->live_fault_g = g_from;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_debug_kernel_counts(const demcz_handle* h, int64_t* counts)
{
    NOT_DERIVED(h);
    if (!h || !counts) return DEMCZ_ERR_INVALID_ARGUMENT;
    const bool wave = h->lanes == DEMCZ_LAYOUT_SPLIT && h->split_kind == SPLIT_WAVE;
    counts[0] = h->kernel_counts[0];
    counts[1] = wave ? h->launches - h->kernel_counts[0] : 0;
    counts[2] = wave ? 0 : h->launches;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_debug_kernel_name(const demcz_handle* h, char* buf, int32_t cap)
{
    NOT_DERIVED(h);
    if (!h || !buf || cap < 1) return DEMCZ_ERR_INVALID_ARGUMENT;
    const int d = h->cfg.d;
    const char* tg = h->cfg.target_kind == DEMCZ_TARGET_MVNORMAL ? "MVNORMAL" : h->cfg.target_kind == DEMCZ_TARGET_ISO_QUAD ? "ISO_QUAD"
                     : h->cfg.target_kind == DEMCZ_TARGET_LINREG_SSE ? "LINREG_SSE" : h->cfg.target_kind == DEMCZ_TARGET_PROGRAM ? "PROGRAM" : "HOST";
    // what the most recent window launch resolved; before any launch: the kernel of a launch that is not LIVE, untempered, general
    const WindowKernel k = h->last_kernel.threads ? h->last_kernel : window_kernel_of(h, launch_facts(h, nullptr, false));
    const char* lv = k.live ? "true" : "false";
    const char* tm = k.temper ? "true" : "false";
    char tmp[160];
    switch (k.arm) {
    case ARM_LR8S: snprintf(tmp, sizeof tmp, "window_kernel_lr8s<%d, %s>", d, lv); break;
    case ARM_PROGRAM_WAVE: snprintf(tmp, sizeof tmp, "%s<%d, %d, %s, %s> (program)", d <= 5 ? "window_kernel_ps" : "window_kernel_pw", (int)TARGET_PROGRAM, d, lv, tm); break;
    case ARM_PS: snprintf(tmp, sizeof tmp, "window_kernel_ps<%s, %d, %s, %s>", tg, d, lv, tm); break;
    case ARM_PS2: snprintf(tmp, sizeof tmp, "window_kernel_ps2<%s, %d, %s, %s>", tg, d, lv, tm); break;
    case ARM_PS2D: snprintf(tmp, sizeof tmp, "window_kernel_ps2d<%s, %d, %s, %s>", tg, d, lv, tm); break;
    case ARM_PW:
        snprintf(tmp, sizeof tmp, "window_kernel_pw<%s, %d, %s, %s%s>", tg, d, lv, tm,
                 k.pw_form == PW_FORM_MATRIX ? ", true" : k.pw_form == PW_FORM_REGULAR ? ", false, true" : "");
        break;
    case ARM_MLB_REC:
        // (the group-start-mask instantiations are reported without their trailing arguments)
        if (h->mlb_qb > 0 && h->split_lanes == 16) snprintf(tmp, sizeof tmp, "window_kernel_mlb<%s, %d, %d, true, %s, %d>", tg, d, h->split_lanes, lv, h->mlb_qb);
        else snprintf(tmp, sizeof tmp, "window_kernel_mlb<%s, %d, %d, true, %s>", tg, d, h->split_lanes, lv);
        break;
    case ARM_LR16_REC: snprintf(tmp, sizeof tmp, "window_kernel_lr16<%d, true, %s>", d, lv); break;
    case ARM_ML_REC: snprintf(tmp, sizeof tmp, "window_kernel_ml<%s, %d, 16, true, %s>", tg, d, lv); break;
    case ARM_PC8: snprintf(tmp, sizeof tmp, "window_kernel_pc8<%s, %d, %s, %s>", tg, d, lv, tm); break;
    case ARM_MLB: snprintf(tmp, sizeof tmp, "window_kernel_mlb<%s, %d, %d>", tg, d, h->lanes); break;
    case ARM_LR16: snprintf(tmp, sizeof tmp, "window_kernel_lr16<%d, false, false>", d); break;
    case ARM_ML_COOP: snprintf(tmp, sizeof tmp, "window_kernel_ml<%s, %d, %d, false, false, true>", tg, d, h->lanes); break;
    case ARM_ML: snprintf(tmp, sizeof tmp, "window_kernel_ml<%s, %d, %d>", tg, d, h->lanes); break;
    case ARM_SNOOKER:
        if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM) snprintf(tmp, sizeof tmp, "snooker_kernel<%d, %d> (program)", (int)TARGET_PROGRAM, d);
        else if (k.dyn_lds) snprintf(tmp, sizeof tmp, "snooker_kernel_generic<%s>", tg);
        else snprintf(tmp, sizeof tmp, "snooker_kernel<%s, %d>", tg, d);
        break;
    case ARM_CROSSOVER:
        if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM) snprintf(tmp, sizeof tmp, "window_kernel_cr<%d, %d%s> (program)", (int)TARGET_PROGRAM, d, k.adapt ? ", adapt" : "");
        else if (k.dyn_lds) snprintf(tmp, sizeof tmp, "window_kernel_cr_generic<%s%s>", tg, k.adapt ? ", adapt" : "");
        else snprintf(tmp, sizeof tmp, "window_kernel_cr<%s, %d%s>", tg, d, k.adapt ? ", adapt" : "");
        break;
    case ARM_ONE_LANE:
        // Known misreport: a dimension with no specialisation launches window_kernel_generic<TARGET> and is still named
        // window_kernel<TARGET, d, FULL> here (tests and profile scripts match on the string; correcting it is a change of behaviour).
        if (h->cfg.target_kind == DEMCZ_TARGET_PROGRAM) snprintf(tmp, sizeof tmp, "window_kernel<%d, %d, %s> (program)", (int)TARGET_PROGRAM, d, h->full_block ? "true" : "false");
        else snprintf(tmp, sizeof tmp, "window_kernel<%s, %d, %s>", tg, d, h->full_block ? "true" : "false");
        break;
    }
    snprintf(buf, (size_t)cap, "demcz::%s", tmp);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_live_status(const demcz_handle* h, int32_t* live_enabled, int32_t* redos)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (live_enabled) *live_enabled = (h->lanes == DEMCZ_LAYOUT_SPLIT && !h->no_live && h->live_claimed) ? 1 : 0;
    if (redos) *redos = h->live_redos;
    return DEMCZ_OK;
}

// The scatter kernels of a sharded run -- append_gathered_kernel (synchronous exchange) and append_batch_kernel
// (batched exchange) -- applied to a slab the CALLER built in the layout an all-gather over R ranks delivers,
// [R][cnt][d][n_loc] with n_loc = this handle's N: lets a one-GPU box check the index arithmetic for R > 1.
extern "C" int32_t demcz_debug_append_slab(demcz_handle* h, const double* slab, int32_t R, int32_t cnt, int32_t batched)
{
    NOT_DERIVED(h);
    if (!h || !slab || R < 1 || cnt < 1 || (!batched && cnt != 1)) return DEMCZ_ERR_INVALID_ARGUMENT;
    if (!h->has_state) return fail(h, DEMCZ_ERR_STATE, "demcz_debug_append_slab: no state");
    if (h->lag != 0 || !h->pending.empty()) return fail(h, DEMCZ_ERR_STATE, "demcz_debug_append_slab: rows are pending");
    const int64_t N = h->cfg.N, rows = N * R * cnt;
    const int d = h->cfg.d;
    if (h->M_app + rows > h->cfg.Mcap) return fail(h, DEMCZ_ERR_CAPACITY, "demcz_debug_append_slab: Z capacity exceeded");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int32_t rc = ensure_scratch(h, rows * d);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_scratch, slab, (size_t)rows * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int64_t tot = rows * d;
    if (batched)
        hipLaunchKernelGGL(append_batch_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ, h->ZS,
                           h->M_app, (const double*)h->d_scratch, N, (int)R, (int)cnt, d);
    else
        hipLaunchKernelGGL(append_gathered_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->dZ, h->ZS,
                           h->M_app, (const double*)h->d_scratch, N, (int)R, d);
    HIPCHK(h, hipGetLastError());
    SYNCCHK(h, h->stream);
    h->M_app += rows;
    h->M = h->M_app;
    rec_invalidate(h);
    return DEMCZ_OK;
}

extern "C" int32_t demcz_set_kernel_timing(demcz_handle* h, int32_t enabled)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    h->timing = enabled != 0;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_kernel_time(demcz_handle* h, int64_t* launches, double* milliseconds)
{
    NOT_DERIVED(h);
    if (!h) return DEMCZ_ERR_INVALID_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    SYNCCHK(h, h->stream);
    double total = 0.0;
    h->after_launch_ev = nullptr;         // (may be one of the events destroyed below)
    h->series_start_ms.clear(); h->series_dur_ms.clear();
    for (auto& pr : h->timed) {
        float ms = 0.0f, st = 0.0f;
        HIPCHK(h, hipEventElapsedTime(&ms, pr.first, pr.second));
        if (&pr != &h->timed.front()) HIPCHK(h, hipEventElapsedTime(&st, h->timed.front().first, pr.first));   // (an event against itself faults in the runtime)
        // a bracket over k autostop slabs (demcz_run_checked): k entries of equal share -- means, not events
        const int32_t k = h->timed_slabs[(size_t)(&pr - &h->timed.front())];
        for (int32_t i = 0; i < k; ++i) { h->series_start_ms.push_back((double)st + i * ((double)ms / k)); h->series_dur_ms.push_back((double)ms / k); }
        total += ms;
    }
    for (auto& pr : h->timed) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (launches) *launches = h->timed_launches;
    if (milliseconds) *milliseconds = total;
    h->timed.clear();
    h->timed_slabs.clear();
    h->timed_launches = 0;
    return DEMCZ_OK;
}

extern "C" int32_t demcz_get_kernel_time_series(demcz_handle* h, int32_t cap, double* start_ms, double* duration_ms, int32_t* n)
{
    NOT_DERIVED(h);
    if (!h || cap < 0 || !n) return DEMCZ_ERR_INVALID_ARGUMENT;
    const int32_t m = (int32_t)std::min<size_t>(h->series_start_ms.size(), (size_t)cap);
    for (int32_t i = 0; i < m; ++i) {
        if (start_ms) start_ms[i] = h->series_start_ms[i];
        if (duration_ms) duration_ms[i] = h->series_dur_ms[i];
    }
    *n = (int32_t)h->series_start_ms.size();
    return DEMCZ_OK;
}
