"""CPU tier: the worlds of tests/full_update_cases.py are worth running -- from the oracle alone.

The full-update kernels resolve one generation at a time (window_kernel_lr8s one or two: its second column is the generation behind
a rejected one), so what a bit comparison can see of a wrong candidate, a wrong sum or a wrong temperature is the accept / reject
path a chain takes.  The oracle's run of every main world (100 generations, block_cases.schedule) must satisfy:
  1. outcomes: per form, "moved" and "did not move" occur at least three times each, and so does each of the four (previous
     generation's outcome, this one's) pairs;
  2. temperatures matter: every tempered piece, run again by the oracle from the state at its start WITHOUT its temperatures, gives
     a different history for at least three chains;
  3. a chain moves in between 0.25 and 0.75 of its generations.
The four-wave worlds (18 generations) are held to 2 and, like the other edge worlds (25 generations), to an acceptance strictly
between 0.1 and 0.9.  The schedules must plan what they claim by the launch rules (demcz_run_plan.h, restated in
full_update_cases.split_live_launches), the LDS limits of the matrix kernels must follow from the restated formulas, and the planned
names must be exactly the kernels the issue lists."""
import functools

import numpy as np
import pytest

import block_cases as bc
import dimension_cases as dc
import full_update_cases as fc

K = fc.K


def test_the_lds_limits_follow_from_the_formulas():
    """demcz_kernels_lr.h at d = 10: 6656 bytes per group of 64 observations + 6416; the two-generation kernel 35 968 more."""
    for ngrp in (1, 2, 18, 23, 24):
        assert fc.lr16_lds(64 * ngrp) == 6656 * ngrp + 6416 == fc.lr16_lds(64 * ngrp - 63)
        assert fc.lr8s_lds(64 * ngrp) - fc.lr16_lds(64 * ngrp) == 35968
    assert fc.LDS_LIMIT == 163840
    assert (fc.LR16_MAX_OBS, fc.lr16_lds(fc.LR16_MAX_OBS)) == (1472, 159504) and fc.lr16_lds(fc.LR16_MAX_OBS + 1) > fc.LDS_LIMIT
    assert (fc.LR8S_MAX_OBS, fc.lr8s_lds(fc.LR8S_MAX_OBS)) == (1152, 162192) and fc.lr8s_lds(fc.LR8S_MAX_OBS + 1) > fc.LDS_LIMIT
    assert fc.lr16_lds(fc.LR8S_MAX_OBS + 1) <= fc.LDS_LIMIT             # 1153..1472: a split handle runs lr16<10, true, ...>
    assert fc.LR16_MAX_OBS + 1 <= dc.ML_COOP_MAX_OBS                    # 1473 fused: window_kernel_ml's helper-wave form
    assert {n for n, _, _ in fc.LR_LIMITS} == {1152, 1153, 1472, 1473}
    assert {n % 64 for n in fc.NOBS_COUNTS} >= {0, 1, 63} and {n % 16 for n in fc.NOBS_COUNTS} >= {0, 1, 15}


def test_split_live_launches_restates_the_plan():
    """plan_launch by hand, K = 5.  A first call of 10: cold, one launch, which prepares 10 generations for the next call.  A call
    of 30 behind it: 10 are there, so 10, then the rest of the call (20 prepared by the launch before): three launches in all.  A
    call behind a call shorter than K is one launch whatever its length; so is one behind demcz_set_state."""
    assert fc.split_live_launches(fc.pieces_of([(10, False), (30, False)])) == [1, 3]
    assert fc.split_live_launches(fc.pieces_of([(3, False), (30, False)])) == [1, 2]
    assert fc.split_live_launches(fc.pieces_of([(10, False), (30, False)]), cold_behind=(10,)) == [1, 2]
    assert fc.split_live_launches(fc.pieces_of([(12, False), (5, False), (12, True)])) == [1, 2, 4]       # (12 > 5 prepared: 5 + 7)
    assert bc.per_window_launches(fc.pieces_of([(3, True), (10, False), (5, True)])) == [1, 4, 6]


@functools.lru_cache(maxsize=None)
def _all_runs():
    return fc.main_runs() + fc.edge_runs()


def test_the_schedules_plan_every_form_and_a_launch_per_piece():
    assert {p[3] for p in fc.schedule()} == {p[3] for p in fc.pieces_of(fc.EDGE_LENGTHS)} == {p[3] for p in fc.pieces_of(fc.RESUMED_LENGTHS)} == set(fc.FORMS)
    T = fc.zero_temperature_case("mvn4")
    assert {0.0, 1e-300, 1e300} <= set(T["temperature"].tolist()) and {p[3] for p in T["pieces"]} == {bc.LIVE_TEMPERED, bc.SHORT_TEMPERED}
    r = fc.resumed_case("mvn6")
    assert r["pieces"][1][1] == fc.RESUME_AT and fc.RESUME_AT % K != 0
    assert [p[3] for p in fc.pieces_of(fc.FOUR_WAVE_LENGTHS)] == [bc.SHORT_TEMPERED, bc.LIVE_PLAIN, bc.LIVE_TEMPERED]
    seen = set()
    for case, layout, env in _all_runs():
        pieces = case["pieces"]
        if (layout, tuple(pieces)) in seen:
            continue
        seen.add((layout, tuple(pieces)))
        assert pieces[0][0] == 1 and all(a == b + 1 for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]))
        for a, b, tempered, form in pieces:
            assert form == bc.form_of(a, b, tempered, K)
        if layout == "split":
            cold = (fc.RESUME_AT,) if case["name"].startswith("full_resumed") else ()
            assert fc.split_live_launches(pieces, K, cold) == list(range(1, len(pieces) + 1)), case["name"]
            assert fc.last_launch_from(case, layout) == pieces[-1][0]
        else:
            # one launch per K-window touched
            counts = [c for _, c in fc.plan(case, layout, env)]
            assert counts == list(np.cumsum([len({(g - 1) // K for g in range(a, b + 1)}) for a, b, _, _ in pieces])), case["name"]
            g = fc.last_launch_from(case, layout)
            assert pieces[-1][0] <= g <= pieces[-1][1] and (g - 1) // K == (pieces[-1][1] - 1) // K and (g == pieces[-1][0] or (g - 1) % K == 0)


def test_the_planned_names_are_exactly_the_kernels_to_cover():
    ml = {"demcz::window_kernel_ml<MVNORMAL, %d, 8>" % d for d in range(2, 11)}
    ml |= {"demcz::window_kernel_ml<ISO_QUAD, 10, 8>", "demcz::window_kernel_ml<MVNORMAL, 20, 16>"}
    ml |= {"demcz::window_kernel_ml<MVNORMAL, 20, 16, true, %s>" % lv for lv in ("true", "false")}
    assert len(ml) == 13
    lr = {"demcz::window_kernel_lr16<10, false, false>", "demcz::window_kernel_lr16<10, true, true>", "demcz::window_kernel_lr16<10, true, false>",
          "demcz::window_kernel_lr8s<10, true>", "demcz::window_kernel_lr8s<10, false>"}
    one = {"demcz::window_kernel<MVNORMAL, %d, true>" % d for d in (2, 3, 4, 5, 8, 10, 20, 7, 13, 64)}
    one |= {"demcz::window_kernel<ISO_QUAD, 10, true>", "demcz::window_kernel<ISO_QUAD, 7, true>"}
    one |= {"demcz::window_kernel<LINREG_SSE, %d, true>" % d for d in (10, 26, 7)}
    # 1473 observations on sixteen lanes: too many for window_kernel_lr16, few enough for the helper waves
    unfit = {"demcz::window_kernel_ml<LINREG_SSE, 10, 16, false, false, true>"}
    names = fc.kernel_names_planned()
    assert names == ml | lr | one | unfit, sorted(names ^ (ml | lr | one | unfit))
    # each main family reaches its names on the full schedule alone
    main = {n for case, lay, env in fc.main_runs() for n, _ in fc.plan(case, lay, env)}
    assert main == ml | lr | one
    spec = {(fc.WORLDS[w][0], fc.WORLDS[w][1]) for w in fc.ONE_LANE_WORLDS}
    assert sum(fc.one_lane_specialised(k, d) for k, d in spec) == 10 and {k for k, d in spec if not fc.one_lane_specialised(k, d)} == {"mvn", "iso", "lr"}
    # the three handles of B at the limits
    by = {(c["nobs"], lay, env): {n for n, _ in fc.plan(c, lay, env)} for c, lay, env in fc.edge_runs() if c["kind"] == "lr"}
    assert by[1152, "split", ()] == {n for n in lr if "lr8s" in n} and by[1153, "split", ()] == {n for n in lr if "lr16<10, true" in n}
    assert by[1472, "split", ()] == by[1153, "split", ()] and by[1472, "fused", ()] == {"demcz::window_kernel_lr16<10, false, false>"}
    assert by[1473, "fused", ()] == unfit == {dc.lr_kernel_name(10, True, lr16_fits=False)}
    assert by[90, "split", (fc.NO_LR_SPEC,)] == by[1153, "split", ()]


def test_four_wave_populations_fill_the_last_workgroup_partly():
    cus = fc.MI355X_CUS
    for name, sign in [(w, 1) for w in fc.FOUR_WAVE_FUSED] + list(fc.FOUR_WAVE_SPLIT):
        case = fc.four_wave_case(name, sign, cus)
        per_wave = 64 // fc.lanes_of(case)
        assert fc.chain_waves(case) >= 4 * cus                                   # demcz_create: four-wave workgroups
        assert case["N"] % (4 * per_wave) != 0 and case["N"] % per_wave != 0
        assert -(-case["N"] // (4 * per_wave)) == cus + (sign > 0)              # workgroups: one per CU, or one more
        assert case["G"] == 3 * K + 3
    assert {fc.WORLDS[w][1] for w in fc.FOUR_WAVE_FUSED} >= {2, 5, 9, 10, 20}
    assert fc.four_wave_case("mvn5")["N"] == 4 * cus * 8 + 5 and fc.four_wave_case("mvn20", -1)["N"] == 4 * cus * 4 - 3


@pytest.mark.parametrize("world", list(fc.WORLDS))
def test_main_worlds_meet_the_three_conditions(oracle, world):
    case = fc.case_of(world)
    ref = bc.oracle_run(oracle, case)
    assert {p[3] for p in case["pieces"]} == set(fc.FORMS) and case["G"] == 100
    share = ref["changed"].sum() / (case["N"] * case["G"])
    outcomes, pairs = bc.outcome_counts(case, ref), bc.pair_counts(case, ref)
    diffs = bc.untempered_differences(oracle, case, ref)
    print(world, "gamma", case["gamma"], "share moved %.3f" % share, "rarest outcome", min(int(outcomes[f].min()) for f in fc.FORMS),
          "rarest pair", min(int(pairs[f].min()) for f in fc.FORMS), "chains that differ without the temperatures, per tempered piece:", diffs)
    for form in fc.FORMS:
        assert outcomes[form].shape == (2,) and (outcomes[form] >= 3).all(), f"{world}, {form}: moved / did not move {outcomes[form]}"
        assert pairs[form].shape == (1, 2, 2) and (pairs[form] >= 3).all(), f"{world}, {form}: (previous, this) pairs {pairs[form].tolist()}"
    assert len(diffs) == sum(1 for p in case["pieces"] if p[2]) and min(diffs) >= 3, f"{world}: {diffs}"
    assert 0.25 <= share <= 0.75, f"{world}: a chain moves in {share:.3f} of its generations"


@functools.lru_cache(maxsize=None)
def _edge_worlds():
    seen = {}
    for case, _, _ in fc.edge_runs():
        seen.setdefault(case["name"], case)
    return seen


@pytest.mark.parametrize("name", list(_edge_worlds()))
def test_edge_worlds_accept_and_reject(oracle, name):
    case = _edge_worlds()[name]
    ref = bc.oracle_run(oracle, case)
    acc = ref["changed"].sum() / (case["N"] * case["G"])
    print(name, "N", case["N"], "acceptance %.3f" % acc)
    assert 0.1 < acc < 0.9, f"{name}: acceptance {acc:.3f}"
    if name.startswith("full_four_wave"):
        diffs = bc.untempered_differences(oracle, case, ref)
        print(name, "chains that differ without the temperatures, per tempered piece:", diffs)
        assert len(diffs) == 2 and min(diffs) >= 3
