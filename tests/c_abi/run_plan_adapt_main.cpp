// run_plan_adapt_main.cpp -- the launch schedule of a one-lane handle that adapts its crossover class weights
// (demc.jl_amd/csrc/demcz_run_plan.h: RunFacts::adapt_every / adapt_until, LaunchPlan::adapt_after) as a stand-alone program, built
// with -fsanitize=address,undefined and run on its own (tests/test_run_plan_adapt.py).
//
//   run_plan_adapt_main walk FILE    every line of FILE is one call:
//                                      K G_FROM LEN E RNG_OFFSET SNOOKER_EVERY ADAPT_EVERY ADAPT_UNTIL
//                                    For each, "case <line number>" and then one line per window launch, as demcz_run walks the call:
//                                      g w_end snooker adapt_after accumulate nbound
// Exit code 2: a case it cannot read; 3: a launch that made no progress.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <deque>

#include "../../demc.jl_amd/csrc/demcz_run_plan.h"

using namespace demcz;

namespace {
struct PendingRows { int64_t visible_from, M_after; };

int walk(const int64_t* a)
{
    RunFacts f;
    f.K = a[0]; f.E = a[3];
    f.N = 100;
    f.g_to = a[1] + a[2] - 1; f.G = a[2]; f.rng_offset = a[4];
    f.hist = true;
    f.snooker_every = a[5]; f.adapt_every = a[6]; f.adapt_until = a[7];
    const std::deque<PendingRows> pending;       // (read for split layouts only)
    for (int64_t g = a[1]; g <= f.g_to;) {
        const LaunchPlan p = plan_launch(f, g, 0, 1000, 1000, RecDesc{}, pending);
        std::printf("%" PRId64 " %" PRId64 " %d %d %d %" PRId64 "\n", p.g, p.w_end, (int)p.snooker, (int)p.adapt_after,
                    (int)adapt_accumulates(f, g), p.nbound);
        if (p.g != g || p.w_end < g || p.w_end > f.g_to) return 3;
        g = p.w_end + 1;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "walk")) {
        std::FILE* in = std::fopen(argv[2], "r");
        if (!in) return 2;
        int rc = 0;
        for (int64_t line = 0; rc == 0; ++line) {
            int64_t a[8];
            int got = 0;
            while (got < 8 && std::fscanf(in, "%" SCNd64, &a[got]) == 1) ++got;
            if (got == 0) break;
            if (got < 8 || a[0] < 1 || a[1] < 1 || a[2] < 1 || a[3] < 0 || a[4] < 0 || a[5] < 0 || a[6] < 0 ||
                (a[6] > 0 && (a[7] < a[6] || a[7] % a[6] != 0))) { rc = 2; break; }
            std::printf("case %" PRId64 "\n", line);
            rc = walk(a);
        }
        std::fclose(in);
        return rc;
    }
    std::fprintf(stderr, "usage: %s walk FILE\n", argv[0]);
    return 2;
}
