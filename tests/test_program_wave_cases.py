"""CPU tier: the worlds of tests/program_wave_cases.py are worth running -- from the oracle, or the oracle's loop around the
Python twin, alone.

A bit comparison sees a wrong candidate, or a wrong log-density, of node n of a pass's tree only where a chain's realised accept /
reject path goes through node n; on the program layout lane n hands candidate n to the user's function.  So the reference's run of
every main world (MvNormal as a program at every d = 2..32, the isotropic quadratic at five dimensions, Rosenbrock at four) must
show
  * every one of the 32 outcomes of a five-generation pass at least three times in the full passes of EACH of the four forms
    (LIVE / non-LIVE x plain / tempered);
  * for every length L = 1..4, plain and tempered separately, every one of the 2^L outcomes at least three times over the run and
    at least once in a pass of that length inside a LIVE launch;
  * temperatures that matter: every tempered piece, run again from the state at its start without them, changes the history of at
    least three chains;
and the worlds with K = 1, 3, 4, 7, 12 every outcome of every pass length they produce.  The schedules must plan what they claim by
the launch rules in program_wave_cases' docstring, the Rosenbrock chains must move in 0.3 .. 0.7 of their generations, and the
restated MvNormal must compile for the wave layout without a device.  (Compiling it at all 31 dimensions, and Rosenbrock at its
four, took 108 s where this was written, nothing cached -- more than a CPU test should: six dimensions are compiled here, and every
dimension by the GPU tier, a handle per d.)"""
import time

import numpy as np
import pytest

import demc_jl_amd as demc
import dimension_cases as dc
import program_wave_cases as pc
from demc_jl_amd import _lib


def _name(kind, d):
    return "%s-%d" % (kind, d)


MAIN_IDS = [_name(k, d) for k, d in pc.MAIN_WORLDS]


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------
def test_the_schedule_tiles_the_run_and_plans_every_form():
    pieces, K = pc.schedule(), pc.K
    assert pieces[0][0] == 1 and pieces[-1][1] <= pc.G_MAX
    assert all(a == b + 1 for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]))
    assert {p[3] for p in pieces} == set(pc.FORMS)
    before = K                                              # (a first call has no draws prepared for it)
    for a, b, tempered, form in pieces:
        n = b - a + 1
        live = (b - 1) // K > (a - 1) // K
        assert form == pc.form_of(a, b, tempered) == "%s %s" % ("LIVE" if live else "non-LIVE", "tempered" if tempered else "plain")
        assert n <= 1024                                    # a call's temperatures lie in the arena (arena_gens)
        if n >= K:
            assert before < K                               # every long piece follows a piece shorter than K: one launch
        if not live:
            assert (a - 1) // K == (b - 1) // K             # inside one K-window
        before = n
    case = pc.mvn_case(6)
    assert pc.launch_pieces(case) == pieces and pc.launches_after(case) == list(range(1, len(pieces) + 1))
    # the pieces the schedule starts from, and the window pairs
    assert [p[:2] for p in pieces[:11]] == [p[:2] for p in dc.pw_schedule()[:11]]
    assert [p[2] for p in pieces[:11]] == [False if i == 1 else p[2] for i, p in enumerate(dc.pw_schedule()[:11])]
    cuts = {((a - 1) % K, b - a + 1) for a, b, _, f in pieces if f.startswith("non")}
    assert {(0, 2), (2, 5), (7, 3), (0, 1), (1, 5), (6, 4)} <= cuts
    for form in pc.FORMS:
        full = sum(1 for a, b, _, f in pieces if f == form for p, q in dc.passes_of(a, b) if q - p == 4)
        assert full >= 8, form
        for L in (1, 2, 3, 4):                              # passes of every length inside and outside LIVE launches, either kind
            assert sum(1 for a, b, _, f in pieces if f == form for p, q in dc.passes_of(a, b) if q - p + 1 == L) >= 2, (form, L)
    # a LIVE piece that starts s before a boundary and ends e behind it: passes of s and e
    assert pc._pieces(pc.crossing(3, 4, True))[1][:2] == (8, 14) and dc.passes_of(8, 14) == [(8, 10), (11, 14)]


def test_the_planned_kernel_names_are_the_four_per_dimension():
    names = pc.kernel_names_planned()
    tf = ("true", "false")
    want = {"demcz::window_kernel_%s<4, %d, %s, %s> (program)" % ("ps" if d <= 5 else "pw", d, l, t) for d in range(2, 33) for l in tf for t in tf}
    assert len(want) == 4 * 31 and names == want, sorted(names ^ want)
    assert pc.kernel_name(5, pc.LIVE_TEMPERED) == "demcz::window_kernel_ps<4, 5, true, true> (program)"
    assert pc.kernel_name(6, pc.SHORT_PLAIN) == "demcz::window_kernel_pw<4, 6, false, false> (program)"


def test_the_worlds_take_their_sizes_from_the_siblings():
    import small_wave_cases as sw
    assert len(pc.MAIN_WORLDS) == 31 + 5 + 4 and [d for k, d in pc.MAIN_WORLDS if k == "mvn"] == list(range(2, 33))
    for d in (2, 3, 4, 5):
        c = pc.mvn_case(d)
        assert (c["N"], c["gamma"], c["seed"]) == (192, sw.GAMMA[d], sw.small_case(d, False)["seed"])
    for d in (6, 11, 19, 32):
        c, s = pc.mvn_case(d), dc.pw_case("mvn", d)
        # the sibling's seed, and its jump but for d = 6..10; 192 chains, not its 96
        assert (c["N"], c["gamma"], c["seed"]) == (192, sw.PC8_GAMMA["mvn", 6] if d == 6 else 0.2, s["seed"])
    for d in pc.ISO_DIMS:
        assert pc.iso_case(d)["gamma"] == (dc.PW_GAMMA["iso"] if d >= 6 else pc.ISO_GAMMA[d]) and pc.iso_case(d)["seed"] != pc.mvn_case(d)["seed"]
    for kind, d in pc.MAIN_WORLDS:
        c = pc.main_case(kind, d)
        assert c["N"] <= 192 and c["G"] <= pc.G_MAX and c["K"] == 10 and c["live"]
    r = pc.rosenbrock_case(6)
    assert r["program"]().data is None or len(r["program"]().data) == 0          # data = NULL, ndata = 0


def test_the_edge_schedules_plan_what_they_name():
    import small_wave_cases as sw
    edges = pc.edge_worlds()
    assert len({m()["name"] for m in edges.values()}) == len(edges)
    for d, N in pc.TINY:
        c = pc.tiny_case(d, N)
        assert {p[3] for p in c["pieces"]} == set(pc.FORMS) and pc.launches_after(c) == [1, 2, 3, 4]
    assert {N for _, N in pc.TINY} == {1, 3, 5, 9} and {d for d, _ in pc.TINY} == {3, 7}
    c = pc.largest_case()
    assert c["N"] == 2048 and c["d"] == 5 and c["G"] == 25 and not c["live"]
    assert pc.launch_pieces(c) == [(1, 10, False, pc.SHORT_PLAIN), (11, 13, False, pc.SHORT_PLAIN), (14, 20, True, pc.SHORT_TEMPERED),
                                   (21, 25, True, pc.SHORT_TEMPERED)]
    assert pc.launches_after(c) == [2, 4]
    for d in pc.OTHER_K_DIMS:
        for k, (lengths, passes) in pc.OTHER_K.items():
            c = pc.other_k_case(d, k)
            assert c["K"] == k and 56 <= c["G"] <= 64 and c["gamma"] != 2.38
            assert [p[3] for p in c["pieces"]] == [pc.LIVE_PLAIN, pc.LIVE_TEMPERED] and pc.launches_after(c) == [1, 2]
            (a0, b0, _, _), (a1, b1, _, _) = c["pieces"]
            assert b1 - a1 <= b0 - a0 and b0 % k == 0      # the second call is no longer than the first: not cut; from a window's start
            assert {q - p + 1 for a, b, _, _ in c["pieces"] for p, q in dc.passes_of(a, b, k)} == set(passes)
    assert dc.passes_of(1, 14, 7) == [(1, 5), (6, 7), (8, 12), (13, 14)] and dc.passes_of(1, 12, 12) == [(1, 5), (6, 10), (11, 12)]
    for d in pc.CUT_DIMS:
        c = pc.cut_case(d)
        assert c["K"] == 5 and pc.launches_after(c) == sw.CUT_LAUNCHES
        assert pc.launch_pieces(c) == [(1, 15, False, pc.LIVE_PLAIN), (16, 30, True, pc.LIVE_TEMPERED), (31, 60, True, pc.LIVE_TEMPERED)]
        assert (31 - 16) % 2 == 1                           # the second launch's temperatures: an odd offset into the call's array
    for d in pc.EDGE_TEMPERATURE_DIMS:
        c = pc.edge_temperature_case(d)
        assert {0.0, 1e-300, 1e300, 2.5} <= set(c["temperature"].tolist()) and [p[3] for p in c["pieces"]] == [pc.LIVE_TEMPERED]
    for d in pc.NO_HISTORY_DIMS:
        assert not pc.no_history_case(d)["history"]
    for d in pc.RESUMED_DIMS:
        c = pc.resumed_case(d)
        assert c["pieces"][1][1] == pc.RESUME_AT and pc.RESUME_AT % c["K"] != 0 and {p[3] for p in c["pieces"]} == set(pc.FORMS)
        assert pc.launches_after(c) == [1, 2, 3, 4, 5, 6]   # (the twelve generations behind the hand-back: nothing prepared, one launch)


def test_launch_pieces_cuts_by_the_rules():
    case = dict(K=10, live=True, resume_at=None, pieces=pc._pieces([(20, False), (45, True), (45, False), (3, False), (30, True)]))
    assert [l[:2] for l in pc.launch_pieces(case)] == [(1, 20), (21, 40), (41, 65), (66, 110), (111, 113), (114, 143)]
    assert pc.launches_after(case) == [1, 3, 4, 5, 6]
    case["live"] = False
    assert pc.launches_after(case)[:2] == [2, 7] and all("non-LIVE" in l[3] for l in pc.launch_pieces(case))


# ---- the conditions, per main world ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", pc.MAIN_WORLDS, ids=MAIN_IDS)
def test_every_outcome_of_every_pass_length_occurs_and_temperatures_matter(oracle, kind, d):
    case = pc.main_case(kind, d)
    ref = pc.reference_run(oracle, case)
    moved = ref["changed"].sum() / (case["N"] * case["G"])
    full = dc.pass_outcomes(case["pieces"], ref["log_obj"], ref["lp0"], forms=pc.FORMS)
    print(case["name"], "gamma", case["gamma"], "a chain moves in %.3f of its generations;" % moved, "rarest outcome of a full pass per form",
          {f: int(full[f].min()) for f in pc.FORMS})
    for form in pc.FORMS:
        missing = [format(o, "05b") for o in range(32) if full[form][o] < 3]
        assert not missing, f"{case['name']}, {form}: outcomes of a full pass seen fewer than three times: {missing}"
    for L in (1, 2, 3, 4):
        c = pc.short_pass_outcomes(case, ref["log_obj"], ref["lp0"], L)
        for tempered in ("plain", "tempered"):
            total, live = c["LIVE " + tempered] + c["non-LIVE " + tempered], c["LIVE " + tempered]
            print(case["name"], "passes of", L, tempered, "rarest outcome over the run", int(total.min()), "inside LIVE launches", int(live.min()))
            assert total.min() >= 3, f"{case['name']}: {tempered} passes of {L}: an outcome seen fewer than three times over the run"
            assert live.min() >= 1, f"{case['name']}: {tempered} passes of {L}: an outcome never seen inside a LIVE launch"
    if kind == "rosenbrock":
        assert 0.3 <= moved <= 0.7
    diffs = pc.untempered_differences(oracle, case, ref)
    assert len(diffs) == sum(1 for p in case["pieces"] if p[2]) >= 1
    print(case["name"], "chains that differ without the temperatures, per tempered piece:", diffs)
    assert min(diffs) >= 3, f"{case['name']}: a tempered piece in which the temperatures change fewer than three chains: {diffs}"


@pytest.mark.parametrize("d", pc.ROSENBROCK_DIMS)
def test_the_twin_loop_in_pieces_is_the_twin_loop_in_one(oracle, d):
    """program_wave_cases.twin_run carries helpers.oracle_sample_logobj on from piece to piece: over untempered pieces that is one
    call of it over the whole stretch."""
    from helpers import oracle_sample_logobj, same_bits
    case = pc.rosenbrock_case(d)
    pieces = [(1, 7, False, ""), (8, 13, False, ""), (14, 30, False, ""), (31, 31, False, "")]
    got = pc.twin_run(oracle, case, pieces=pieces)
    w = case["problem"]
    ref = oracle_sample_logobj(oracle, case["logobj"], w["Zinit"], case["N"], case["K"], 31, None, w["eps_scale"], case["gamma"], case["seed"])
    same_bits(got, ref, what=case["name"])
    assert got["M"] == ref["M"] and np.array_equal(got["changed"], ref["changed"])


# ---- the edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", list(pc.OTHER_K))
@pytest.mark.parametrize("d", pc.OTHER_K_DIMS)
def test_other_window_lengths_show_every_outcome_of_their_passes(oracle, d, k):
    case = pc.other_k_case(d, k)
    ref = pc.reference_run(oracle, case)
    for L in pc.OTHER_K[k][1]:
        c = dc.pass_outcomes(pc.launch_pieces(case), ref["log_obj"], ref["lp0"], k=k, forms=pc.FORMS, length=L)
        assert not c[pc.SHORT_PLAIN].any() and not c[pc.SHORT_TEMPERED].any()
        total = c[pc.LIVE_PLAIN] + c[pc.LIVE_TEMPERED]
        print(case["name"], "passes of", L, "rarest outcome", int(total.min()))
        assert total.min() >= 1, f"{case['name']}: passes of {L}: an outcome never seen"
    assert min(pc.untempered_differences(oracle, case, ref)) >= 3


def test_the_edge_worlds_accept_and_reject_and_their_temperatures_matter(oracle):
    for name, make in pc.edge_worlds().items():
        case = make()
        if name.startswith("K"):
            continue                                        # (the test above)
        ref = pc.reference_run(oracle, case)
        moved = ref["changed"].sum() / (case["N"] * case["G"])
        diffs = pc.untempered_differences(oracle, case, ref)
        print(name, "a chain moves in %.3f of its generations; chains that differ without the temperatures:" % moved, diffs)
        assert 0.1 < moved < 0.9, name
        if not name.startswith("tiny"):
            assert min(diffs) >= 3, name
    tiny = [pc.untempered_differences(oracle, c, pc.reference_run(oracle, c)) for c in (pc.tiny_case(d, N) for d, N in pc.TINY)]
    assert sum(max(t) >= 1 for t in tiny) >= len(tiny) // 2       # (one to nine chains: in half of these worlds at least)


# ---- the programs compile for the wave layout without a GPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 5, 6, 13, 20, 32])
def test_mvnormal_compiles_for_the_wave_layout(d):
    """d = 2, 5: window_kernel_ps; 6, 13, 20, 32: window_kernel_pw (the module's docstring: why not every d here)."""
    t0 = time.perf_counter()
    pc.mvn_case(d)["program"]().check(layout=_lib.LAYOUT_PROGRAM_WAVE)
    print("d = %d: the wave unit compiled in %.1f s" % (d, time.perf_counter() - t0))
    assert _lib.LAYOUT_PROGRAM_WAVE == demc.LAYOUT_PROGRAM_WAVE
