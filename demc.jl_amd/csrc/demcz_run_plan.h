// demcz_run_plan.h -- the window launches one demcz_run call is cut into: where a launch ends, whether it is
// a LIVE one, whether a two-chain handle may take its regular kernel, how far the draw records let it go, and what the launch
// after it will look like.  Plain C++, no HIP calls: demcz_capi.hip executes the plan, and tests/c_abi/run_plan_main.cpp walks
// whole calls with it as a stand-alone program (tests/test_run_plan.py).
#pragma once

#include <algorithm>
#include <cstdint>

#include "demcz_slab_plan.h"

namespace demcz {

// ---- K boundaries ------------------------------------------------------------------------------------------------------------------
// the first multiple of K that is >= g
inline int64_t boundary_at_or_after(int64_t g, int64_t K) { return ((g - 1) / K + 1) * K; }
// multiples of K inside g..e
inline int64_t boundaries_in(int64_t g, int64_t e, int64_t K) { return e / K - (g - 1) / K; }

// A regular launch of a kernel that runs R generations per pass (PS_R, PS2_R): K, the distance to the first boundary and the
// length are multiples of R, and the launch is at least one pass long.
inline bool regular_passes(int64_t K, int64_t to_boundary, int64_t ngen, int64_t R)
{
    return K % R == 0 && to_boundary % R == 0 && ngen % R == 0 && ngen >= R;
}

// The joint history (chain and log_obj in one allocation) of N chains, d parameters and Gcap generations, in bytes; window_kernel_ps2
// / ps2d reach it by 32-bit offsets while it stays below the limit.
inline double hist_joint_bytes(int64_t N, int d, int64_t Gcap) { return (double)N * (d + 1) * (double)Gcap * 8.0; }
inline bool hist_offsets_32bit(int64_t N, int d, int64_t Gcap) { return hist_joint_bytes(N, d, Gcap) < 4293918720.0; }
inline uint32_t hist_bytes_u32(int64_t N, int d, int64_t Gcap) { return (uint32_t)std::min<double>(hist_joint_bytes(N, d, Gcap), 4294967295.0); }

// ---- deferred appends (lag E > 0) -----------------------------------------------------------------------------------------------------
// boundary j belongs to the batch closing at J = ceil(j / E) * E; its rows are drawn from generation (J + E) * K + 1 on -- the same
// rule on every rank and for any sharding
inline int64_t lag_batch_of(int64_t j, int64_t E) { return ((j + E - 1) / E) * E; }
inline int64_t lag_visible_from(int64_t J, int64_t E, int64_t K) { return (J + E) * K + 1; }

// ---- draw records ------------------------------------------------------------------------------------------------------------------
// What a record buffer holds: draws of generations g_first .. g_first + ngen - 1 (positions of the random streams), their row
// indices drawn against M rows + `rows` more per boundary passed, the first boundary K - boff generations in.
struct RecDesc {
    bool valid = false;
    int64_t g_first = 0, M = 0, rows = 0;
    int32_t ngen = 0, boff = 0;
    // the row indices in a record were drawn against M + (boundaries passed) * rows: all of that must agree
    bool serves(int64_t g_first_, int64_t ngen_, int64_t M_, int64_t rows_, int32_t boff_) const
    {
        return valid && g_first == g_first_ && ngen >= ngen_ && M == M_ && rows == rows_ && boff == boff_;
    }
};

// the span a launch whose draws have to be made first is held to: whole K-windows of COLD_REC_MIB (twice that for a two-chain handle)
inline int64_t cold_start_limit(int64_t K, int64_t rec_bytes_per_gen, bool two_chain)
{
    return std::max<int64_t>(K, ((int64_t)((two_chain ? 2 * COLD_REC_MIB : COLD_REC_MIB) << 20) / rec_bytes_per_gen / K) * K);
}

// ---- one call -----------------------------------------------------------------------------------------------------------------------
// what is fixed over one demcz_run call
struct RunFacts {
    int64_t K = 1;
    int64_t E = 0;                  // append lag, in batches of K-windows
    bool external_append = false;   // the caller appends (and a call crosses at most one boundary, at its end)
    int64_t N = 0, shards = 1;      // chains of this handle; replicas whose rows join the archive
    bool peer = false;              // the rows of all shards arrive inside the launches: every launch is of the LIVE kind
    int64_t g_to = 0, G = 0;        // the call's last generation and its length
    int64_t rng_offset = 0;
    bool split = false;             // split layout: a launch's producer half prepares the next launch's draws
    bool hist = false;              // a history is kept
    // a two-chain handle (R generations per pass) and what its regular launches need beyond regular passes: everything reachable
    // through the arena
    bool two_chain = false;
    int64_t R = 1;
    bool temp_in_arena = true;      // (or no temperatures)
    bool hist_32bit = true;
    bool arena = false, rec_in_arena = false;
    int64_t cold_limit = 0;         // cold_start_limit
    int64_t next_hint = 0;          // generations of the launch that follows the call (0: not known -- taken to be as long as this call)
    bool force_live = false;        // diagnosis: the LIVE instantiation also for launches with no boundary inside
    int64_t snooker_every = 0;      // s >= 1: generation g is a snooker generation when (g + rng_offset) % s == 0 (0: none)
    // adaptation of the crossover class weights (demcz_set_crossover_adapt): the weights are updated behind every generation g with
    // (g + rng_offset) % adapt_every == 0 and g + rng_offset <= adapt_until (0: none; adapt_until % adapt_every == 0)
    int64_t adapt_every = 0, adapt_until = 0;
};

struct LaunchPlan {
    int64_t g = 0, w_end = 0;       // the launch runs generations g .. w_end
    int64_t to_boundary = 0;        // generations up to and including the first K boundary at or after g
    int64_t nbound = 0;             // boundaries inside the launch
    bool live = false;              // generations of this launch draw from rows appended inside it
    bool dual = false;              // a two-chain handle's regular launch
    // split layouts: the launch after this one, whose draws this launch's producer half prepares
    int64_t next_g_first = 0, next_ngen = 0, next_M = 0, next_rows = 0;
    int32_t next_boff = 0;
    bool snooker = false;           // the launch is one snooker generation (snooker_kernel, demcz_kernels_snooker.h)
    bool adapt_after = false;       // the launch ends on an update position of the class weights: cr_adapt_kernel follows it
};

// ---- snooker generations -------------------------------------------------------------------------------------------------------------
// The same number positions the Philox streams, so a resumed run (rng_offset) makes the choices an uninterrupted one would.
inline bool snooker_generation(const RunFacts& f, int64_t g) { return f.snooker_every > 0 && (g + f.rng_offset) % f.snooker_every == 0; }
// the first snooker generation at or after g (callers ask only with snooker_every > 0)
inline int64_t snooker_at_or_after(const RunFacts& f, int64_t g)
{
    const int64_t s = f.snooker_every, r = (g + f.rng_offset) % s;
    return r == 0 ? g : g + (s - r);
}

// ---- adaptation of the crossover class weights -------------------------------------------------------------------------------------
// generation g lies at or in front of `until` (stream numbering, as the snooker rule's): its crossover steps are accumulated
inline bool adapt_accumulates(const RunFacts& f, int64_t g) { return f.adapt_every > 0 && g + f.rng_offset <= f.adapt_until; }
// the first update position at or after g, as a generation of the call (callers ask only where adapt_accumulates(f, g): it is
// then at or in front of `until`, itself an update position)
inline int64_t adapt_update_at_or_after(const RunFacts& f, int64_t g)
{
    const int64_t e = f.adapt_every, r = (g + f.rng_offset) % e;
    return r == 0 ? g : g + (e - r);
}

// The launch that starts at generation g.  `span`: what live_span() says a LIVE launch may cover (0: no LIVE launches); M, M_app:
// rows proposals draw from and rows appended, BEFORE the rows pending at g are admitted; cur: the descriptor of the record buffer
// this launch reads; pending: (visible_from, M_after) in the order of their visibility.  (static: an instantiation adds nothing to the symbols the library exports)
template <class Pending>
static LaunchPlan plan_launch(const RunFacts& f, int64_t g, int64_t span, int64_t M, int64_t M_app, const RecDesc& cur, const Pending& pending)
{
    const int64_t K = f.K, E = f.E;
    LaunchPlan p;
    p.g = g;
    const int64_t next_boundary = boundary_at_or_after(g, K);
    p.to_boundary = next_boundary - g + 1;
    const int64_t rest = f.g_to - g + 1;
    // Synchronous schedule: a launch ends at the next K boundary, the kernel boundary is the
    // grid-wide barrier before the new rows are drawn from.  Deferred schedule: nothing appended
    // inside a batch becomes visible inside it, so one launch covers the rest of the batch.
    int64_t w_end = std::min(next_boundary, f.g_to);
    if (E > 0 && !f.external_append) w_end = std::min(lag_batch_of(next_boundary / K, E) * K, f.g_to);
    // Split layout on one GPU: the launch runs on through the boundaries; waves hand the appended rows
    // to each other inside it (LIVE, demcz_kernels_pc.h), so the schedule is still the synchronous one.
    if (f.two_chain) {
        // A two-chain handle runs its REGULAR launches (start, boundary distance and length multiples of five; everything
        // reachable through the arena) on window_kernel_ps2d; anything else takes the general kernel, one chain per wave, and
        // -- twice the waves: they would not all be resident -- never across a K boundary.
        p.dual = regular_passes(K, p.to_boundary, rest - rest % f.R, f.R) && f.temp_in_arena && (!f.hist || f.hist_32bit) && f.arena && f.rec_in_arena;
        if (!p.dual) span = 0;
        else if (span > 0) span = std::max<int64_t>((std::min(span, rest) / f.R) * f.R, f.R);
        else w_end = g + ((w_end - g + 1) / f.R) * f.R - 1;       // (a K-window cut short by the call's end: whole passes only)
    }
    if (span > 0) {
        // How far this launch goes: as far as the records allow -- but no further than the draws that ARE there, where the
        // launch before prepared fewer than that (a call longer than the last one); and a launch whose draws have to be made
        // first, with nothing to run beside (the first of a run), stays short: its producer is serial time
        // (64 MiB of records, the span of every launch until round 3f; profiles/r03f_launch_span.txt).
        int64_t n = std::min(span, rest);
        const int64_t rows_v = f.N * (f.peer ? f.shards : 1);      // (live: immediate visibility; all shards' rows with peers)
        if (cur.serves(g + f.rng_offset, K, M, rows_v, (int32_t)(K - p.to_boundary))) {
            if (cur.ngen < n) n = std::max<int64_t>((cur.ngen / K) * K, K);
        } else {
            n = std::min(n, f.cold_limit);
        }
        if (p.dual) n = std::max<int64_t>((n / f.R) * f.R, f.R);
        w_end = g + n - 1;
    }
    // Snooker generations are launches of their own: the move is the same for all chains of a generation and known here, so
    // no window kernel has to know of it.  (One-lane handles only: span == 0, no split, no two-chain regularity to keep.)
    if (f.snooker_every > 0) {
        if (snooker_generation(f, g)) { w_end = g; p.snooker = true; }
        else w_end = std::min(w_end, snooker_at_or_after(f, g) - 1);
    }
    // The class weights change behind an update position, so a launch ends at the first one at or after g -- whatever kind of
    // generation stands there, and K boundaries or not (a deferred-append launch over several K-windows is cut as well).
    if (adapt_accumulates(f, g)) {
        const int64_t u = adapt_update_at_or_after(f, g);
        w_end = std::min(w_end, u);
        p.adapt_after = w_end == u;
    }
    p.w_end = w_end;
    p.nbound = boundaries_in(g, w_end, K);
    // boundaries whose rows generations of this same launch draw from.  With peers EVERY launch is of the LIVE kind: the rows
    // of the boundary that ended the launch before may still be on their way from another replica's publisher
    p.live = span > 0 && (boundaries_in(g, w_end - 1, K) > 0 || f.peer || f.force_live);
    if (f.split) {
        // what the launch after this one will be, so that this launch's producer half can prepare
        // its draws: it starts at w_end + 1, runs to its own boundary / batch end / span, and sees ...
        const int64_t ng = w_end + 1;
        const int64_t nb1 = boundary_at_or_after(ng, K);       // its first boundary
        const int64_t nend = (E > 0 && !f.external_append) ? lag_batch_of(nb1 / K, E) * K : nb1;
        const int64_t rows_n = f.N * f.shards;
        p.next_M = M;
        p.next_ngen = nend - ng + 1;
        // a next call is taken to be as long as this one -- unless demcz_run_checked knows what follows
        if (span > 0) p.next_ngen = std::min(span, (w_end < f.g_to) ? f.g_to - w_end : (f.next_hint > 0 ? f.next_hint : f.G));
        if (f.external_append) p.next_ngen = 0;                      // the caller appends: M is not ours to predict
        else if (E == 0) p.next_M = M_app + p.nbound * rows_n;                    // ... the rows appended now
        else for (const auto& pe : pending) if (pe.visible_from <= ng) p.next_M = pe.M_after;   // ... or admitted by then
        p.next_rows = (E == 0) ? rows_n : 0;      // rows that join per boundary passed inside a launch (this one's and the next's alike)
        p.next_g_first = ng + f.rng_offset;
        p.next_boff = (int32_t)(K - (nb1 - ng + 1));
    }
    return p;
}

}  // namespace demcz
