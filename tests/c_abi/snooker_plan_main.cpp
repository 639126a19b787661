// snooker_plan_main.cpp -- demcz_run's launch schedule with snooker generations (demc.jl_amd/csrc/demcz_run_plan.h: RunFacts::
// snooker_every, LaunchPlan::snooker) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run
// on its own (tests/test_snooker_plan.py).  One-lane handles: no span, no split, no two-chain regularity.
//
//   snooker_plan_main walk FILE    every line of FILE is one call:  K G_FROM LEN EVERY RNG_OFFSET E EXTERNAL
//                                  For each, "case <line number>" and then one line per launch, as demcz_run walks the call:
//                                    g w_end to_boundary nbound snooker
// Exit code 3: a launch made no progress.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <deque>

#include "../../demc.jl_amd/csrc/demcz_run_plan.h"

using namespace demcz;

namespace {
constexpr int64_t N = 70, M0 = 110;
struct PendingRows { int64_t visible_from, M_after; };

int walk(const int64_t* a)
{
    const int64_t K = a[0], g_from = a[1], len = a[2], E = a[5];
    RunFacts f;
    f.K = K; f.E = E; f.external_append = a[6] != 0;
    f.N = N; f.g_to = g_from + len - 1; f.G = len; f.rng_offset = a[4];
    f.hist = true;
    f.snooker_every = a[3];
    int64_t M = M0, M_app = M0, batch_J = -1;
    std::deque<PendingRows> pending;
    const RecDesc none;
    for (int64_t g = g_from; g <= f.g_to;) {
        const LaunchPlan p = plan_launch(f, g, 0, M, M_app, none, pending);
        std::printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", p.g, p.w_end, p.to_boundary, p.nbound, (int)p.snooker);
        if (p.g != g || p.w_end < g || p.w_end > f.g_to) return 3;
        while (!pending.empty() && pending.front().visible_from <= g) { M = pending.front().M_after; pending.pop_front(); }
        if (p.nbound > 0 && !f.external_append) {
            if (E == 0) {
                M_app += p.nbound * N;
                M = M_app;
            } else {
                for (int64_t j = (g - 1) / K + 1; j <= p.w_end / K; ++j) {
                    const int64_t J = lag_batch_of(j, E);
                    M_app += N;
                    if (batch_J != J) { pending.push_back({lag_visible_from(J, E, K), M_app}); batch_J = J; }
                    else pending.back().M_after = M_app;
                }
            }
        }
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
            int64_t a[7];
            int got = 0;
            while (got < 7 && std::fscanf(in, "%" SCNd64, &a[got]) == 1) ++got;
            if (got == 0) break;
            if (got < 7 || a[0] < 1 || a[1] < 1 || a[2] < 1 || a[3] < 0 || a[4] < 0 || a[5] < 0) { rc = 2; break; }
            std::printf("case %" PRId64 "\n", line);
            rc = walk(a);
        }
        std::fclose(in);
        return rc;
    }
    std::fprintf(stderr, "usage: %s walk FILE\n", argv[0]);
    return 2;
}
