// demcz_slab_plan.h -- how long a LIVE launch of an arena handle may be, and which autostop slabs of a demcz_run_checked call go
// into one demcz_run call: plain C++, no HIP calls, so that it also builds into a stand-alone program
// (tests/c_abi/slab_plan_main.cpp).
//
//   arena_span:      the archive, two draw-record buffers and a call's temperatures lie in ONE allocation that window_kernel_ps2 /
//                    ps2d reach by 32-bit offsets, so its size stays below ARENA_LIMIT.  The record buffers take `target_bytes`
//                    each; an archive that leaves less room gets shorter buffers, down to 4 K generations -- below that no arena.
//   slab_group_end:  with nothing decided per slab (threshold <= 0) consecutive slabs run as one demcz_run call, i.e. as few
//                    launches as the span allows, and their checks as one batch beside the next group.  At the default span
//                    that joins slabs shorter than half of it: 1000-generation slabs at C2 stay one call and one launch each.
#pragma once

#include <cstdint>

namespace demcz {

constexpr uint64_t ARENA_LIMIT = 0xF0000000ull;          // bytes: everything in the arena is reached by a 32-bit offset
constexpr int64_t SPAN_GENS_MAX = (int64_t)1 << 20;      // generations of one launch, whatever the buffers would hold
// Record bytes per buffer of an arena handle (twice that for a two-chain handle: up to twice the chains).  C2 (1024 chains,
// d = 5: 57 344 B per generation): 1170 generations, one autostop slab of 1000 and no second one.  Measured against about 2000,
// 5000 and 10 000 generations per launch: none of them is faster at C2 (profiles/r10_launch_span.txt) -- the producer beside a
// launch makes 1000 generations of draws in 85-110 us while the launch runs them in 130, so a launch that is to be longer than
// the one before it waits for its draws.  DEMCZ_REC_MIB sets another size (measurements).
constexpr int64_t ARENA_REC_MIB = 64;
// the span a launch whose draws have to be made first is held to (the first of a run), whatever the buffers' size
constexpr int64_t COLD_REC_MIB = 64;

struct ArenaSpan {
    int64_t gens;        // generations each record buffer holds; 0: no arena
    int64_t span;        // generations a LIVE launch may cover (before the history window bounds it)
    uint64_t zb, rb, tb; // bytes of the archive, of one record buffer, of the temperatures (each a multiple of 256)
};

inline uint64_t arena_total(const ArenaSpan& a) { return a.zb + 2 * a.rb + a.tb; }

inline void arena_sizes(ArenaSpan& a, uint64_t zbytes, int64_t N, int d, int64_t rec_pad)
{
    a.zb = (zbytes + 255) & ~(uint64_t)255;
    a.rb = (((uint64_t)a.gens * (uint64_t)(d + 2) * (uint64_t)N + (uint64_t)rec_pad) * 8 + 255) & ~(uint64_t)255;
    a.tb = (((uint64_t)a.gens + 64) * 8 + 255) & ~(uint64_t)255;
}

// zbytes: the archive (Mcap rows); Gcap: the history window (0: none kept, launches are as long as a call); rec_pad: doubles
// behind a record buffer.
inline ArenaSpan arena_span(uint64_t zbytes, int64_t N, int d, int64_t K, int64_t Gcap, int64_t target_bytes, int64_t rec_pad)
{
    ArenaSpan a{0, 0, 0, 0, 0};
    const int64_t per_gen = (int64_t)(d + 2) * N * 8;
    int64_t span = target_bytes / per_gen;
    if (span > SPAN_GENS_MAX) span = SPAN_GENS_MAX;
    if (span < K) span = K;
    auto gens_of = [&](int64_t s) {
        int64_t g = s;
        if (Gcap > 0 && g > (Gcap > 1024 ? Gcap : 1024)) g = (Gcap > 1024 ? Gcap : 1024);
        if (g < 4 * K) g = 4 * K;
        return g;
    };
    a.gens = gens_of(span);
    arena_sizes(a, zbytes, N, d, rec_pad);
    if (arena_total(a) >= ARENA_LIMIT) {
        // the longest buffers that fit: first by division, then exactly
        const uint64_t fixed = ((zbytes + 255) & ~(uint64_t)255) + 2 * ((uint64_t)rec_pad * 8 + 256) + (64 * 8 + 256);
        if (fixed >= ARENA_LIMIT) return ArenaSpan{0, 0, 0, 0, 0};
        int64_t fit = (int64_t)((ARENA_LIMIT - fixed) / (2 * (uint64_t)per_gen + 8));
        if (fit > span) fit = span;
        for (;; --fit) {
            if (fit < 4 * K || fit < 1) return ArenaSpan{0, 0, 0, 0, 0};
            a.gens = fit;
            arena_sizes(a, zbytes, N, d, rec_pad);
            if (arena_total(a) < ARENA_LIMIT) break;
        }
        for (; fit < span; ++fit) {         // (the division allowed for the most padding there can be)
            a.gens = fit + 1;
            arena_sizes(a, zbytes, N, d, rec_pad);
            if (arena_total(a) >= ARENA_LIMIT) break;
        }
        span = fit;
        a.gens = gens_of(span);        // (never more than `fit`: the history window only shortens it, and fit >= 4 K)
        arena_sizes(a, zbytes, N, d, rec_pad);
    }
    a.span = span;
    return a;
}

// ---- groups of slabs ---------------------------------------------------------------------------------------------------------------
// Slab ends are the multiples of `every`; a call g_from..g_to may start and end inside a slab.
//
// The check of a group is one batch of three launches on the side stream, beside the next group's window launch -- the stream
// that launch's producer is on as well.  Only the batch of the group in front of the call's last slab is waited for at the end of
// the call, and it must be over before that slab's launch is.  Measured at C2 (1024 chains, d = 5, every = 1000;
// profiles/r10_launch_span.txt): one slab's check 33 us (history re-read 13, the two small kernels 9 + 10, the copy 5), the
// producer of the next call's first 1000 generations 87-92 us, the last slab's window launch 130-140 us.  33 + 90 fits beside it;
// a second slab's check does not.  Re-read and launch both grow with `every`, the rest does not.
constexpr int SLAB_TAIL_GROUP_MAX = 1;
// (a batch's scratch is one slice per slab -- the caller passes fewer where 64 slices would be large --, and a grid's z extent is bounded)
constexpr int SLAB_GROUP_MAX = 64;

inline int64_t slab_end_at_or_after(int64_t g, int64_t every) { return ((g + every - 1) / every) * every; }

// The last generation of the group that starts at g (g_from <= g <= g_to):
//   * it ends on a slab end, or at g_to;
//   * the call's last slab -- the one that holds g_to -- is a group of its own;
//   * from its first slab end on it covers at most `span` generations (a first slab longer than that stands alone) and at most
//     max_slabs (1..SLAB_GROUP_MAX) slabs;
//   * `cut` > g: it does not reach past the first slab end e with e + 1 >= cut, so that a launch starts there (the debug hook's
//     generation; the generation a redo goes LIVE again behind).  cut <= g: no such point ahead.
//   * the group in front of the last slab has at most SLAB_TAIL_GROUP_MAX slabs.
inline int64_t slab_group_end(int64_t g, int64_t g_to, int64_t every, int64_t span, int64_t cut, int64_t max_slabs = SLAB_GROUP_MAX)
{
    const int64_t e1 = slab_end_at_or_after(g, every);
    if (e1 >= g_to) return g_to;
    const int64_t last_start = ((g_to - 1) / every) * every + 1;      // first generation of the slab that holds g_to
    const int64_t lim = last_start - 1;                                // (a slab end, >= e1)
    int64_t e = lim;
    if (span < e - g + 1) e = ((g + span - 1) / every) * every;        // (span: any positive value, INT64_MAX for "no bound")
    if (max_slabs < 1) max_slabs = 1;
    if (max_slabs > SLAB_GROUP_MAX) max_slabs = SLAB_GROUP_MAX;
    if ((e - e1) / every + 1 > max_slabs) e = e1 + (max_slabs - 1) * every;
    if (cut > g) {
        const int64_t ec = slab_end_at_or_after(cut - 1, every);
        if (e > ec) e = ec;
    }
    if (e < e1) e = e1;
    if (e == lim && (e - e1) / every + 1 > SLAB_TAIL_GROUP_MAX) e = lim - (int64_t)SLAB_TAIL_GROUP_MAX * every;
    return e;
}

// slab ends inside g..e (e from slab_group_end)
inline int64_t slab_ends_in(int64_t g, int64_t e, int64_t every) { return e / every - (g - 1) / every; }

}  // namespace demcz
