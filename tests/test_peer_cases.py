"""CPU tier: the replica-group worlds of tests/peer_cases.py are worth running -- from the oracle alone.

A group differs from a single handle in where a boundary's rows land (row_off + cl of brows = N_total) and in who writes the rows
a wave waits for.  A bit comparison sees a row that landed in a neighbour's place, or a sentinel read as data, only when a later
block-step DRAWS that row; and a row that is never drawn only in the archive comparison.  So the oracle's draws alone must give
  * the hand-off: in a main run every ordered pair of different ranks has, per LIVE form, at least 8 block-steps of a generation
    bK + 1 in which the reader draws a row the writer appended at boundary b (both generations inside one piece of that form:
    the row is handed over inside the launches); in a shard-shape or edge run at least one over the run;
  * in every run, for every member, a row it appended that no later step draws.
The plans: every main run reaches every form of its family, every planned kernel name is one the single-handle suites plan, and
the launches of every run are those the executable planner (demcz_run_plan.h through tests/c_abi/run_plan_main.cpp, built as
tests/test_run_plan.py builds it) makes of the same calls with `peer` set."""
import pytest

import block_cases as bc
import dimension_cases as dc
import full_update_cases as fc
import peer_cases as pc
import small_wave_cases as sw
from test_run_plan import Case, Launch, program          # noqa: F401  (the fixture that builds and runs the planner)

MAIN = pc.main_runs() + [pc.l32_run()]
HANDOFF = [r for r in pc.all_runs() if r["handoff"]]
SPAN, COLD = 1170, 11980                  # longer than any piece


def _live_forms(run):
    return [f for f in pc.FAMILY_FORMS[run["family"]] if "non-LIVE" not in f]


def _single_handle_names():
    pw = {dc.pw_kernel_name(kind, d, f) for kind, dims in (("mvn", dc.PW_DIMS), ("iso", dc.PW_DIMS)) for d in dims for f in dc.FORMS}
    return sw.kernel_names_planned() | pw | bc.kernel_names_planned() | fc.kernel_names_planned()


def test_every_main_run_reaches_every_form_and_every_name_is_a_known_one():
    known = _single_handle_names()
    for run in MAIN:
        assert {p[3] for p in run["case"]["pieces"]} == set(pc.FAMILY_FORMS[run["family"]]), run["id"]
        assert run["case"]["N"] == run["R"] * run["n_loc"]
    names = pc.kernel_names_planned()
    assert names <= known, sorted(names - known)
    assert not any("ps2d" in n for n in names), "a member of a group never runs two chains to a wave"
    main = pc.kernel_names_planned(MAIN)
    print("kernel names the group runs plan (%d, %d of them in the main runs):" % (len(names), len(main)))
    for n in sorted(names):
        print("   ", n, "" if n in main else "(lockstep or edge runs only)")
    tf = ("true", "false")
    want = {"demcz::%s<MVNORMAL, %d, true, %s>" % (k, d, t) for k in ("window_kernel_ps", "window_kernel_ps2") for d in sw.DIMS for t in tf}
    want |= {dc.pw_kernel_name(kind, d, f) for kind, dims in (("mvn", dc.PW_DIMS), ("iso", pc.PW_ISO_DIMS)) for d in dims
             for f in (dc.REG_PLAIN, dc.REG_TEMPERED, dc.LIVE_PLAIN, dc.LIVE_TEMPERED)}
    # every LIVE REC form of window_kernel_mlb that block_cases plans, the 32-lane one included (a member runs no non-LIVE form)
    want |= {bc.reported_name(i) for i in bc.instantiations_planned() if i[2] and i[3]}
    want |= {"demcz::window_kernel_ml<MVNORMAL, 20, 16, true, true>", "demcz::window_kernel_lr16<10, true, true>", "demcz::window_kernel_lr8s<10, true>"}
    assert main == want, sorted(main ^ want)
    # the instantiations behind the reported names of window_kernel_mlb: ungrouped, group-start mask, incremental on 8 and 16 lanes;
    # on 32 lanes the one world the switch is asked for (four blocks of five there run the group-start mask, not the incremental form)
    inst = {bc.instantiation(r["case"], "split", "LIVE plain", lanes=32 if pc.L32 in r["env"] else None) for r in MAIN if r["family"] == "mlb"}
    assert inst == {i for i in bc.instantiations_planned() if i[2] and i[3] and i[1] != 32} | {(20, 32, True, True, 0, True)}, sorted(inst)


def test_the_small_schedules_plan_every_form():
    assert {p[3] for p in sw._pieces(pc.K10_EDGE_LENGTHS, sw.form_of)} == set(sw.ONE_FORMS)
    assert {p[3] for p in sw._pieces(pc.K10_EDGE_LENGTHS, dc.form_of)} == set(dc.FORMS)
    assert sum(n for n, _ in pc.K10_EDGE_LENGTHS) == 50 and sum(n for n, _ in bc.EDGE_LENGTHS) == 25
    zero = {p[3] for p in sw._pieces(pc.K10_ZERO_LENGTHS, sw.form_of)}
    assert zero == {sw.STEADY_LIVE_TEMPERED, sw.STEADY_SHORT_TEMPERED, sw.GENERAL_LIVE_TEMPERED, sw.GENERAL_SHORT_TEMPERED}
    shapes = pc.shape_runs()
    assert {(r["n_loc"], r["R"]) for r in shapes} == set(pc.SHAPE_N_LOC)
    for run in shapes:
        case = run["case"]
        assert case["problem"]["Zinit"].shape[0] <= case["N"] + max(pc.ARCHIVE_EXTRA, 0) or case["problem"]["Zinit"].shape[0] == case["N"]
        assert {p[3] for p in case["pieces"]} == set(pc.FAMILY_FORMS[run["family"]]), run["id"]
    # the chains per workgroup of every publishing site (PS_CHAINS = 4 waves; 64 / L chains a wave, wpw waves; 16 and 8 of the
    # matrix kernels): no n_loc of the shard shapes is a multiple of any
    for n_loc, _ in pc.SHAPE_N_LOC:
        assert all(n_loc % per_wg for per_wg in (4, 8, 16, 32)), n_loc
    for run in pc.edge_runs():
        if run["resume_at"]:
            assert run["resume_at"] % run["case"]["K"] != 0 and any(p[1] == run["resume_at"] for p in run["case"]["pieces"])
    assert [r["id"] for r in pc.edge_runs() if not r["history"]] == ["no_history pw mvn d6", "no_history mlb d5_gm"]


def test_a_members_launches_are_cut_as_a_single_split_handles():
    assert pc.counts_behind(pc.member_walk(bc.pieces_of(sw.CUT_LENGTHS, sw.CUT_K), sw.CUT_K)[0]) == sw.CUT_LAUNCHES
    assert pc.member_walk(bc.pieces_of([(15, False), (45, True)], 5), 5)[0] == [[(1, 15)], [(16, 30), (31, 60)]]
    assert pc.counts_behind(pc.lockstep_walk(bc.pieces_of([(3, True), (10, False)]), 5)) == [1, 4]
    for run in HANDOFF:
        case = run["case"]
        cold = (run["resume_at"],) if run["resume_at"] else ()
        walk, _ = pc.member_walk(case["pieces"], case["K"], cold)
        assert pc.counts_behind(walk) == fc.split_live_launches(case["pieces"], case["K"], cold), run["id"]
        assert pc.counts_behind(walk) == list(range(1, len(case["pieces"]) + 1)), f"{run['id']}: a piece is one launch: the name read behind it is that launch's"
    for run in pc.lockstep_runs():
        assert pc.counts_behind(pc.lockstep_walk(run["case"]["pieces"], run["case"]["K"])) == bc.per_window_launches(run["case"]["pieces"], run["case"]["K"])


def _planner_case(run, piece, at_hand):
    """The call `piece` of a member as tests/c_abi/run_plan_main.cpp reads it.  The draws at hand (as many generations as the call
    before was long) are the program's DESC: fewer than K serve no K-window (0: none at hand); as many as the call or more: 1; K
    of them under a longer call: 2.  No other case occurs in these schedules."""
    a, b = piece[:2]
    K, n = run["case"]["K"], b - a + 1
    if not run["handoff"]:
        # group_execute: plan_launch's schedule without a span
        return Case(K, a, n, 0, 0, 0, 1, 0, int(run["layout"] >= 100), 0, 0, 0, 0, 0, 0, 3 * K, 0)
    desc = 0 if at_hand < K else 1 if at_hand >= n else 2 if at_hand == K else None
    assert desc is not None, (run["id"], piece, at_hand)
    return Case(K, a, n, 0, SPAN, 0, run["R"], 1, 1, 0, 0, desc, 0, 0, 0, COLD, 0)


def test_the_plans_launches_are_the_executable_planners(program):
    run_program, tmp = program
    cases, want = [], []
    for run in pc.all_runs():
        case = run["case"]
        if run["handoff"]:
            walk, at_hand = pc.member_walk(case["pieces"], case["K"], (run["resume_at"],) if run["resume_at"] else ())
        else:
            walk, at_hand = pc.lockstep_walk(case["pieces"], case["K"]), [0] * len(case["pieces"])
        for piece, launches, p in zip(case["pieces"], walk, at_hand):
            cases.append(_planner_case(run, piece, p))
            want.append((run["id"], piece, launches, run["handoff"]))
    (tmp / "peer_cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    walks = []
    for line in run_program("walk", tmp / "peer_cases.txt").splitlines():
        if line.startswith("case "):
            walks.append([])
        else:
            walks[-1].append(Launch(*(int(x) for x in line.split())))
    assert len(walks) == len(cases) > 1000
    for (rid, piece, launches, handoff), got in zip(want, walks):
        assert [(p.g, p.w_end) for p in got] == launches, (rid, piece)
        assert all(p.live == int(handoff) and not p.dual for p in got), f"{rid}, {piece}: every launch of a member is of the LIVE kind"
    # and the same count behind every piece as the plan the GPU tier asserts
    for run in pc.all_runs():
        counts = [c for _, c in pc.plan(run)[0]]
        assert counts[-1] == sum(len(w[2]) for w in want if w[0] == run["id"]), run["id"]


@pytest.mark.parametrize("run", HANDOFF, ids=pc.ids(HANDOFF))
def test_the_handoff_matters_and_some_row_is_never_drawn(oracle, run):
    case, R = run["case"], run["R"]
    counts = pc.handoff_counts(oracle, case, R)
    left = pc.never_drawn(oracle, case, R)
    pairs = [(r, w) for r in range(R) for w in range(R) if r != w]
    forms = _live_forms(run) + [pc.ACROSS_CALLS]
    print(run["id"], "forms", sorted({p[3] for p in case["pieces"]}))
    for r, w in pairs:
        print("    rank %d draws rank %d's fresh rows:" % (r, w), {f: counts.get((r, w, f), 0) for f in forms}, "steps")
    print("    rows appended and never drawn again, per member:", left)
    if run["kind"] == "main":
        for r, w in pairs:
            for f in _live_forms(run):
                assert counts.get((r, w, f), 0) >= 8, f"{run['id']}: rank {r} draws rank {w}'s fresh rows in {counts.get((r, w, f), 0)} steps of {f}"
    else:
        for r, w in pairs:
            assert sum(counts.get((r, w, f), 0) for f in forms) >= 1, f"{run['id']}: rank {r} never draws a row rank {w} has just appended"
    assert min(left) >= 1, f"{run['id']}: a member all of whose appended rows are drawn again: {left}"
