"""CPU tier: the worlds of tests/small_wave_cases.py are worth running -- from the oracle alone.

As in tests/test_dimension_cases.py a bit comparison sees a wrong candidate add or a wrong node log-density of a pass's tree only
on a realised path through that node.  So for d = 2..5 the oracle's run of each schedule must show EVERY one of the 32 outcomes of
a five-generation pass in the full passes of EACH form (eight with one chain to a wave, six with two), each at least three times
over the run; with two chains to a wave the same separately for the even- and the odd-indexed chains, the two halves of a wave;
and in the general kernel's passes of 1..4 generations every one of the 2, 4, 8, 16 outcomes, separately plain and tempered.  The
schedules must plan what they claim by the launch rules in small_wave_cases' docstring.  The replicated consumer resolves one
generation at a time: its worlds must accept between 0.2 and 0.8 of the proposals.

Kernel names asserted by tests/test_gpu_small_wave.py, derived below from the case tables: 16 window_kernel_ps2, 16
window_kernel_ps2d, 16 window_kernel_ps (d = 2..5 x LIVE x TEMPER each) and 40 window_kernel_pc8."""
import numpy as np
import pytest

import dimension_cases as dc
import small_wave_cases as sw


_WORLDS = {}


def _world(oracle, d, dual):
    """The case and the oracle's run of it, computed once."""
    if (d, dual) not in _WORLDS:
        case = sw.small_case(d, dual)
        _WORLDS[d, dual] = case, dc.oracle_run(oracle, case)
    return _WORLDS[d, dual]


@pytest.mark.parametrize("dual", [False, True], ids=["one", "dual"])
def test_the_schedules_tile_the_run_and_plan_every_form(dual):
    pieces = sw.dual_schedule() if dual else sw.one_schedule()
    forms = sw.DUAL_FORMS if dual else sw.ONE_FORMS
    K = sw.K
    assert pieces[0][0] == 1 and pieces[-1][1] == 500
    for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]):
        assert a == b + 1
    assert {p[3] for p in pieces} == set(forms)
    before = K                                              # (a first call has no draws prepared for it)
    for a, b, tempered, form in pieces:
        n = b - a + 1
        steady, live = form.startswith("steady"), "non-LIVE" not in form
        assert form.endswith("tempered" if tempered else "plain")
        assert n <= 1024                                    # a call's temperatures lie in the arena (arena_gens)
        assert steady == sw.regular(a, b)
        if steady:
            assert K % 5 == 0 and (K - (a - 1) % K) % 5 == 0 and n % 5 == 0 and n >= 5
        if live:
            assert (b - 1) // K > (a - 1) // K              # a generation behind a boundary
            assert before < K                               # one launch: nothing prepared that would cut it
        launches = sw.dual_launches(a, b)
        if dual:
            assert {l[2] for l in launches} == {steady}     # every launch of the piece runs the same kernel
            if steady:
                assert launches == [(a, b, True, live)]
            else:
                assert not live and len(launches) == (b - 1) // K - (a - 1) // K + 1       # one launch per K-window
                assert all((q - 1) // K == (p - 1) // K for p, q, _, _ in launches)
        elif not live:
            assert (a - 1) // K == (b - 1) // K             # inside one K-window
        if not steady and not dual:
            assert live or (a - 1) % 5 != 0 or n % 5 != 0
        before = n
    for form in forms:                                      # about forty generations' worth of full passes per form
        full = sum(1 for a, b, _, f in pieces if f == form for p, q in dc.passes_of(a, b) if q - p == 4)
        assert full >= 8, form
    for tempered in (False, True):                          # the general kernel's shorter passes
        for L in (1, 2, 3, 4):
            assert any(q - p + 1 == L for a, b, t, f in pieces if t == tempered and f.startswith("general") for p, q in dc.passes_of(a, b))
    if dual:                                                # a general piece of two launches
        assert any(len(sw.dual_launches(a, b)) == 2 for a, b, _, f in pieces if f.startswith("general"))
        assert sw.dual_launches(8, 13) == [(8, 10, False, False), (11, 13, False, False)]
        assert sw.dual_launches(11, 50) == [(11, 50, True, True)] and sw.dual_launches(6, 10) == [(6, 10, True, False)]
        assert sw.dual_launches(1, 43) == [(1, 40, True, True), (41, 43, False, False)]


def test_every_instantiation_appears_in_a_planned_kernel_name():
    names = sw.kernel_names_planned()
    tf = ("true", "false")
    for fn in ("window_kernel_ps2", "window_kernel_ps2d", "window_kernel_ps"):
        want = {"demcz::%s<MVNORMAL, %d, %s, %s>" % (fn, d, l, t) for d in sw.DIMS for l in tf for t in tf}
        assert len(want) == 16 and want <= names, sorted(want - names)
    want = {"demcz::window_kernel_pc8<%s, %d, %s, %s>" % (dc.TARGET_NAME[k], d, l, t) for k, d in sw.PC8_TARGETS for l in tf for t in tf}
    assert len(want) == 40 and want <= names, sorted(want - names)
    assert len(names) == 16 + 16 + 16 + 40


def test_pass_outcomes_takes_forms_a_length_and_chains():
    """Three chains, one general piece of generations 1..3 (one pass of three): chain 0 moves in 1, chain 1 in 2 and 3, chain 2 never."""
    lp0 = np.zeros(3)
    lo = np.array([[1.0, 1.0, 1.0], [0.0, 2.0, 3.0], [0.0, 0.0, 0.0]])
    pieces = [(1, 3, False, sw.GENERAL_SHORT_PLAIN)]
    c = dc.pass_outcomes(pieces, lo, lp0, forms=sw.GENERAL_FORMS, length=3)
    assert c[sw.GENERAL_SHORT_PLAIN].tolist() == [1, 0, 0, 1, 1, 0, 0, 0]
    c = dc.pass_outcomes(pieces, lo, lp0, forms=sw.GENERAL_FORMS, length=3, chains=np.array([1]))
    assert c[sw.GENERAL_SHORT_PLAIN].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert not dc.pass_outcomes(pieces, lo, lp0, forms=sw.GENERAL_FORMS)[sw.GENERAL_SHORT_PLAIN].any()       # no full pass


@pytest.mark.parametrize("d", sw.DIMS)
@pytest.mark.parametrize("dual", [False, True], ids=["one", "dual"])
def test_every_outcome_of_a_pass_occurs_in_every_form_and_half(oracle, dual, d):
    case, ref = _world(oracle, d, dual)
    forms = sw.DUAL_FORMS if dual else sw.ONE_FORMS
    assert case["K"] == 10 and case["pieces"][-1][1] == case["G"] and case["N"] % 2 == int(dual)
    acc = ref["changed"].sum() / (case["N"] * case["G"])
    for half, chains in sw.halves(case).items():
        counts = dc.pass_outcomes(case["pieces"], ref["log_obj"], ref["lp0"], forms=forms, chains=chains)
        total = sum(counts.values())
        print("dual" if dual else "one", d, half, {f: int(v.min()) for f, v in counts.items()}, "over the run:", int(total.min()),
              "acceptance %.3f" % acc)
        for form in forms:
            missing = [format(o, "05b") for o in range(32) if counts[form][o] < 1]
            assert not missing, f"d = {d}, {half} chains, {form}: outcomes never seen: {missing}"
        assert total.min() >= 3


@pytest.mark.parametrize("d", sw.DIMS)
@pytest.mark.parametrize("dual", [False, True], ids=["one", "dual"])
def test_every_outcome_of_the_general_kernels_shorter_passes_occurs(oracle, dual, d):
    case, ref = _world(oracle, d, dual)
    for L in (1, 2, 3, 4):
        counts = dc.pass_outcomes(case["pieces"], ref["log_obj"], ref["lp0"], forms=sw.GENERAL_FORMS, length=L)
        for tempered in ("plain", "tempered"):
            c = sum(v for f, v in counts.items() if f.endswith(tempered))
            print("dual" if dual else "one", d, "passes of", L, tempered, "minimum", int(c.min()))
            missing = [format(o, "0%db" % L) for o in range(1 << L) if c[o] < 1]
            assert not missing, f"d = {d}, {tempered} passes of {L}: outcomes never seen: {missing}"


def test_the_pc8_schedule_plans_every_form():
    pieces = sw.pc8_schedule()
    K = sw.K
    assert pieces[0][0] == 1 and all(a == b + 1 for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]))
    assert {p[3] for p in pieces} == set(sw.PC8_FORMS)
    before = K
    for a, b, tempered, form in pieces:
        assert form.endswith("tempered" if tempered else "plain")
        if form.startswith("LIVE"):
            assert (b - 1) // K > (a - 1) // K + 1 and before < K       # crosses boundaries, one launch
        else:
            assert (a - 1) // K == (b - 1) // K
        before = b - a + 1


@pytest.mark.parametrize("kind,d", sw.PC8_TARGETS)
def test_pc8_worlds_accept_and_reject(oracle, kind, d):
    case = sw.pc8_case(kind, d)
    ref = dc.oracle_run(oracle, case)
    acc = ref["changed"].sum() / (case["N"] * case["G"])
    print(kind, d, "acceptance %.3f" % acc)
    assert 0.2 < acc < 0.8
