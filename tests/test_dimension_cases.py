"""CPU tier: the worlds of tests/dimension_cases.py are worth running -- from the oracle alone.

A bit comparison of a wave-per-chain kernel with the oracle sees a wrong candidate add for generation u in some lane, or a wrong
log-density of some node of a pass's tree, only where a chain's realised path goes through that node: an ancestor's candidate
matters on the paths that accepted it, a node's own on the paths that reach it.  So for every (target, d) the oracle's run of the
schedule must show EVERY one of the 32 accept / reject outcomes of a five-generation pass in the passes of EACH of the six forms,
and each at least three times over the run.  The regression worlds must accept and reject, and their observation counts must hold
the three kinds of round the helper waves distinguish."""
import numpy as np
import pytest

import dimension_cases as dc


def test_the_schedule_tiles_the_run_and_plans_every_form():
    pieces = dc.pw_schedule()
    assert pieces[0][0] == 1
    for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]):
        assert a == b + 1
    assert {p[3] for p in pieces} == set(dc.FORMS)
    K = dc.K
    before = K                                              # (a first call has no draws prepared for it)
    for a, b, tempered, form in pieces:
        n, live = b - a + 1, "non-LIVE" not in form
        assert ("tempered" in form) == tempered
        if form in (dc.REG_PLAIN, dc.REG_TEMPERED):
            assert K % 5 == 0 and (K - (a - 1) % K) % 5 == 0 and n % 5 == 0
        if live:
            assert (b - 1) // K > (a - 1) // K              # a generation behind a boundary
            assert before < K                               # one launch: nothing prepared that would cut it (the module's docstring)
            if form in (dc.LIVE_PLAIN, dc.LIVE_TEMPERED):
                assert (a - 1) % K != 0 or n % 5 != 0
        else:
            assert (a - 1) // K == (b - 1) // K             # inside one K-window
        before = n
    # the passes: five generations, cut at the boundaries and at the end
    assert dc.passes_of(149, 191) == [(149, 150)] + [(g, g + 4) for g in range(151, 190, 5)] + [(191, 191)]
    assert dc.passes_of(101, 143)[-2:] == [(136, 140), (141, 143)]
    assert dc.passes_of(56, 95) == [(g, g + 4) for g in range(56, 95, 5)]
    for form in dc.FORMS:                                   # about forty generations' worth of full passes per form
        full = sum(1 for a, b, _, f in pieces if f == form for p, q in dc.passes_of(a, b) if q - p == 4)
        assert full >= 8, form


def test_pass_outcomes_counts_what_it_says():
    """Two chains, one REG piece of two passes: the first chain moves in generations 1 and 7, the second in all but 5."""
    lp0 = np.array([0.0, 0.0])
    lo = np.zeros((2, 10))
    lo[0, 0:] = 1.0
    lo[0, 6:] = 2.0
    lo[1] = [1, 2, 3, 4, 4, 5, 6, 7, 8, 9]
    pieces = [(1, 10, False, dc.REG_PLAIN)]
    c = dc.pass_outcomes(pieces, lo, lp0)
    want = np.zeros(32, dtype=np.int64)
    for code in (0b10000, 0b01000, 0b11110, 0b11111):
        want[code] += 1
    assert np.array_equal(c[dc.REG_PLAIN], want)
    assert all(not c[f].any() for f in dc.FORMS if f != dc.REG_PLAIN)


@pytest.mark.parametrize("d", dc.PW_DIMS)
@pytest.mark.parametrize("kind", ["mvn", "iso"])
def test_every_outcome_of_a_pass_occurs_in_every_form(oracle, kind, d):
    case = dc.pw_case(kind, d)
    assert case["K"] == 10 and case["pieces"][-1][1] == case["G"]
    ref = dc.oracle_run(oracle, case)
    counts = dc.pass_outcomes(case["pieces"], ref["log_obj"], ref["lp0"])
    total = sum(counts.values())
    print(kind, d, {f: int(v.min()) for f, v in counts.items()}, "over the run:", int(total.min()))
    for form in dc.FORMS:
        missing = [format(o, "05b") for o in range(32) if counts[form][o] < 1]
        assert not missing, f"{kind} d = {d}, {form}: outcomes never seen: {missing}"
    assert total.min() >= 3


def test_resident_tiles_restate_the_header():
    """ml_coop_resident_tiles against the constants' text in demcz_kernels_ml.h (so that a changed header is noticed here)."""
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "demc.jl_amd" / "csrc" / "demcz_kernels_ml.h").read_text()
    assert re.search(r"#define ML_COOP_RES_BYTES 102400\b", text) and re.search(r"ML_COOP_MAX_OBS = 1536;", text)
    assert "ML_COOP_RES_BYTES / (512 * D)" in text
    assert [dc.ml_coop_resident_tiles(d) for d in (2, 8, 9, 10, 17, 28)] == [24, 24, 22, 20, 11, 7]


@pytest.mark.parametrize("coop", [True, False], ids=["coop", "nocoop"])
@pytest.mark.parametrize("d", dc.LR_DIMS)
def test_regression_worlds_accept_and_reject(oracle, d, coop):
    case = dc.lr_case(d, coop)
    N, K, nobs = case["N"], case["K"], case["nobs"]
    assert N % 4 != 0 and K == 10
    (a0, b0, t0), (a1, b1, t1) = case["pieces"]
    assert a0 == 1 and a1 == b0 + 1 and b1 == case["G"] and b0 % K != 0 and (not t0) and t1       # cut inside a window
    if coop:
        res = dc.ml_coop_resident_tiles(d)
        full = nobs // 64
        assert nobs <= dc.ML_COOP_MAX_OBS
        assert min(res, full) >= 1                                  # resident full rounds
        assert full > res or res >= dc.ML_COOP_MAX_OBS // 64 - 1    # a full round that is not resident, where nobs can hold one
        assert nobs % 64 != 0 and (nobs % 64) % 16 != 0             # a partial last round, no multiple of sixteen
    else:
        assert nobs == 1601 > dc.ML_COOP_MAX_OBS
    ref = dc.oracle_run(oracle, case)
    acc = ref["changed"].sum() / (N * case["G"])
    print(d, coop, nobs, "acceptance %.3f" % acc)
    assert 0.1 < acc < 0.9
