// slab_plan_main.cpp -- the launch-span sizing and the slab grouping of demcz_run_checked (demc.jl_amd/csrc/demcz_slab_plan.h) as a
// stand-alone program, so that they can be built with -fsanitize=address,undefined and run on their own (tests/test_slab_plan.py).
//
//   slab_plan_main groups G_FROM G_TO EVERY SPAN CUT MAX_SLABS   one line "g e" per group, as demcz_run_checked walks the call
//                                                                (SPAN 0: no bound)
//   slab_plan_main arena ZBYTES N D K GCAP TARGET_BYTES REC_PAD  one line "gens span zb rb tb"
//   slab_plan_main consts                                        "ARENA_LIMIT SLAB_TAIL_GROUP_MAX SLAB_GROUP_MAX ARENA_REC_MIB"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../demc.jl_amd/csrc/demcz_slab_plan.h"

static int64_t num(const char* s) { return (int64_t)std::strtoll(s, nullptr, 10); }

int main(int argc, char** argv)
{
    using namespace demcz;
    if (argc == 8 && !std::strcmp(argv[1], "groups")) {
        const int64_t g_from = num(argv[2]), g_to = num(argv[3]), every = num(argv[4]), span = num(argv[5]), cut = num(argv[6]), ms = num(argv[7]);
        if (g_from < 1 || g_to < g_from || every < 1 || span < 0) return 2;
        for (int64_t g = g_from; g <= g_to;) {
            const int64_t e = slab_group_end(g, g_to, every, span > 0 ? span : INT64_MAX, cut, ms);
            std::printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", g, e, slab_ends_in(g, e, every));
            if (e < g) return 3;        // (no progress: the test fails on the exit code)
            g = e + 1;
        }
        return 0;
    }
    if (argc == 9 && !std::strcmp(argv[1], "arena")) {
        const ArenaSpan a = arena_span((uint64_t)std::strtoull(argv[2], nullptr, 10), num(argv[3]), (int)num(argv[4]), num(argv[5]), num(argv[6]),
                                       num(argv[7]), num(argv[8]));
        std::printf("%" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", a.gens, a.span, a.zb, a.rb, a.tb);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "consts")) {
        std::printf("%" PRIu64 " %d %d %" PRId64 "\n", ARENA_LIMIT, SLAB_TAIL_GROUP_MAX, SLAB_GROUP_MAX, ARENA_REC_MIB);
        return 0;
    }
    std::fprintf(stderr, "usage: %s groups|arena|consts ...\n", argv[0]);
    return 2;
}
