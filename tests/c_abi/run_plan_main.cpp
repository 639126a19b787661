// run_plan_main.cpp -- the launch schedule of demcz_run (demc.jl_amd/csrc/demcz_run_plan.h) as a stand-alone program, so that it can
// be built with -fsanitize=address,undefined and run on its own (tests/test_run_plan.py).
//
//   run_plan_main walk FILE    every line of FILE is one call:
//                                K G_FROM LEN E SPAN EXTERNAL SHARDS PEER SPLIT TWO_CHAIN REG_FACTS DESC RNG_OFFSET HINT PENDING COLD FORCE_LIVE
//                              For each, "case <line number>" and then one line per window launch, as demcz_run walks the call:
//                                g w_end to_boundary nbound live dual next_g_first next_ngen next_M next_rows next_boff serves cur_ngen
//                              (serves, cur_ngen: whether the record descriptor at hand serves a K-window at g, and its length)
//                              DESC: 0 invalid, 1 right, 2 right but K generations long, 3 right but for another M.
//                              PENDING: 1: the rows of the boundaries before G_FROM are still pending (two batches; E > 0, G_FROM > K).
//   run_plan_main consts       "N M0 R"
// Exit code 3: a launch made no progress.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <deque>

#include "../../demc.jl_amd/csrc/demcz_run_plan.h"

using namespace demcz;

namespace {
constexpr int64_t N = 100, M0 = 1000, R = 5;
struct PendingRows { int64_t visible_from, M_after; };

int walk(const int64_t* a)
{
    const int64_t K = a[0], g_from = a[1], len = a[2], E = a[3], span = a[4], desc = a[11], pend = a[14];
    RunFacts f;
    f.K = K; f.E = E; f.external_append = a[5] != 0;
    f.N = N; f.shards = a[6]; f.peer = a[7] != 0;
    f.g_to = g_from + len - 1; f.G = len; f.rng_offset = a[12];
    f.split = a[8] != 0; f.hist = true;
    f.two_chain = a[9] != 0; f.R = R;
    f.temp_in_arena = f.hist_32bit = f.arena = f.rec_in_arena = a[10] != 0;
    f.cold_limit = a[15]; f.next_hint = a[13]; f.force_live = a[16] != 0;
    const int64_t rows = N * f.shards;
    int64_t M = M0, M_app = M0, batch_J = -1;
    std::deque<PendingRows> pending;
    const int64_t j0 = (g_from - 1) / K;            // boundaries before the call
    if (pend && E > 0 && j0 >= 1) {
        const int64_t J1 = lag_batch_of(j0, E);
        pending.push_back({lag_visible_from(J1 - E, E, K), M0 + rows});
        pending.push_back({lag_visible_from(J1, E, K), M0 + 2 * rows});
        M_app = M0 + 2 * rows;
        batch_J = J1;
    }
    RecDesc cur;
    if (desc != 0) {
        cur.valid = true;
        cur.g_first = g_from + f.rng_offset;
        cur.M = desc == 3 ? M + 7 : M;
        cur.rows = E == 0 ? rows : 0;
        cur.ngen = (int32_t)(desc == 2 ? K : std::max(span, len));
        cur.boff = (int32_t)(K - (boundary_at_or_after(g_from, K) - g_from + 1));
    }
    for (int64_t g = g_from; g <= f.g_to;) {
        const int64_t tb = boundary_at_or_after(g, K) - g + 1;
        const bool serves = cur.serves(g + f.rng_offset, K, M, N * (f.peer ? f.shards : 1), (int32_t)(K - tb));
        const int32_t cur_ngen = cur.ngen;
        const LaunchPlan p = plan_launch(f, g, span, M, M_app, cur, pending);
        std::printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d\n",
                    p.g, p.w_end, p.to_boundary, p.nbound, (int)p.live, (int)p.dual, p.next_g_first, p.next_ngen, p.next_M, p.next_rows,
                    (int)p.next_boff, (int)serves, (int)cur_ngen);
        if (p.g != g || p.w_end < g) return 3;
        // admit_pending
        while (!pending.empty() && pending.front().visible_from <= g) { M = pending.front().M_after; pending.pop_front(); }
        if (f.split) {
            // pc_prepare: this launch's draws are made now unless the descriptor at hand serves it; the one written for "next" is
            // the one at hand for the launch after this
            const int64_t ngen = p.w_end - g + 1;
            if (!cur.serves(g + f.rng_offset, ngen, M, p.next_rows, (int32_t)(K - p.to_boundary))) {
                cur.valid = true; cur.g_first = g + f.rng_offset; cur.M = M; cur.ngen = (int32_t)ngen; cur.rows = p.next_rows;
                cur.boff = (int32_t)(K - p.to_boundary);
            }
            RecDesc next;
            next.valid = p.next_ngen > 0; next.g_first = p.next_g_first; next.M = p.next_M; next.ngen = (int32_t)p.next_ngen;
            next.rows = p.next_rows; next.boff = p.next_boff;
            cur = next;
        }
        if (p.nbound > 0 && !f.external_append) {
            if (E == 0) {
                M_app += p.nbound * rows;
                M = M_app;
            } else {
                for (int64_t j = (g - 1) / K + 1; j <= p.w_end / K; ++j) {
                    const int64_t J = lag_batch_of(j, E);
                    M_app += rows;
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
            int64_t a[17];
            int got = 0;
            while (got < 17 && std::fscanf(in, "%" SCNd64, &a[got]) == 1) ++got;
            if (got == 0) break;
            if (got < 17 || a[0] < 1 || a[1] < 1 || a[2] < 1 || a[3] < 0 || a[4] < 0 || a[6] < 1) { rc = 2; break; }
            std::printf("case %" PRId64 "\n", line);
            rc = walk(a);
        }
        std::fclose(in);
        return rc;
    }
    if (argc == 2 && !std::strcmp(argv[1], "consts")) {
        std::printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", N, M0, R);
        return 0;
    }
    std::fprintf(stderr, "usage: %s walk FILE | consts\n", argv[0]);
    return 2;
}
