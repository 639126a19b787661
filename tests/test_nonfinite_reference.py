"""The reference and the inputs of test_gpu_nonfinite.py, checked without a GPU.

That file compares every kernel layout with the oracle on populations that hold +-inf, NaN, -0.0, subnormals and values whose
squares overflow, and program targets with a Python driver (helpers.oracle_sample_logobj).  Here:
  * the driver against the oracle itself, on a Python restatement of the isotropic quadratic;
  * the comparison's own strictness (helpers.same_bits sees -0.0 and a NaN in the wrong place, and nothing of a NaN's payload);
  * that the oracle's run of every row of the kernel-choice table, on its poisoned population, has what the GPU test is meant to
    exercise: chains that move, chains that are never finite, `changed` events that are NaN differences, non-finite archive rows;
  * that the three subnormal worlds are subnormal."""
import math
from fractions import Fraction

import numpy as np
import pytest

import demc_jl_amd as demc
import nonfinite_cases as nf
from helpers import (NAN_NEG, NAN_POS, POISON_VALUES, bits_differ, oracle_sample, oracle_sample_logobj, poisoned_population, py_fma,
                     same_bits)
from program_texts import box_closure

TINY = np.finfo(np.float64).tiny


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def test_same_bits_sees_the_sign_of_zero_and_misplaced_nans():
    a = np.array([[0.0, -0.0, 1.5], [np.nan, np.inf, 5e-324]], order="F")
    b = a.copy(order="F")
    assert bits_differ(a, b) is None
    b[1, 0] = _bits(NAN_NEG | 0x1234)                      # another NaN at the same place: sign and payload are not compared
    assert bits_differ(a, b) is None and not np.array_equal(a.view(np.uint64), b.view(np.uint64))
    c = a.copy(order="F")
    c[0, 1] = 0.0
    assert np.array_equal(a[0], c[0]) and "bits differ at (0, 1)" in bits_differ(a, c)
    c = a.copy(order="F")
    c[1, 1] = np.nan
    assert "NaN at (1, 1)" in bits_differ(a, c)
    c = a.copy(order="F")
    c[1, 2] = 0.0
    assert "bits differ at (1, 2)" in bits_differ(a, c)
    assert "shapes" in bits_differ(a, a[:1])
    with pytest.raises(AssertionError, match="X: bits differ"):
        same_bits(dict(X=a), dict(X=-a), keys=("X",))


def test_poisoned_population_holds_every_value_among_chains_and_archive():
    for d, N in ((3, 8), (5, 64), (10, 100)):
        Z = poisoned_population(d, N, 3)
        assert Z.shape == (2 * N + 40, d) and Z.flags.f_contiguous
        assert np.array_equal(Z, poisoned_population(d, N, 3), equal_nan=True)
        clean = np.random.default_rng(3).standard_normal(Z.shape)
        touched = (Z.view(np.uint64) != np.asfortranarray(clean).view(np.uint64))
        assert touched.sum(axis=1).max() == 1
        assert touched[:N + 40].any(axis=1).sum() == (N + 40) // 4 and touched[N + 40:].any(axis=1).sum() == max(1, N // 4)
        assert not (Z.view(np.uint64) == np.uint64(0xFFF4DEADC0DE5EED)).any()             # the library's sentinel is reserved
    want = set(np.array(POISON_VALUES).view(np.uint64).tolist())
    assert len(want) == 14 and {NAN_POS, NAN_NEG, 0x8000000000000000, 1} <= want
    Z = poisoned_population(5, 64, 3)
    for part in (Z[:104], Z[104:]):
        assert want <= set(np.ascontiguousarray(part).view(np.uint64).ravel().tolist())
    assert math.isfinite(1.3e154 * 1.3e154) and math.isinf(1.4e154 * 1.4e154)


# ---- the new driver against the oracle -----------------------------------------------------------------------------------------
def test_py_fma_is_one_rounding():
    assert py_fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60          # (unfused: 2^-29)
    assert (1.0 + 2.0 ** -30) * (1.0 + 2.0 ** -30) - 1.0 == 2.0 ** -29
    assert py_fma(2.0 ** -540, 2.0 ** -534, 5e-324) == 2 * 5e-324                                # subnormal result
    assert py_fma(1e200, 1e200, 0.0) == math.inf and py_fma(-1e200, 1e200, 1e308) == -math.inf
    assert py_fma(1e200, 1e200, -math.inf) == -math.inf and math.isnan(py_fma(math.inf, 0.0, 1.0))
    assert math.isnan(py_fma(math.inf, 1.0, -math.inf)) and math.isnan(py_fma(1.0, math.nan, 1.0))
    assert math.copysign(1.0, py_fma(0.0, -1.0, -0.0)) == -1.0 and math.copysign(1.0, py_fma(3.0, -1.0, 3.0)) == 1.0
    r = np.random.default_rng(0)
    for a, b, c in r.standard_normal((200, 3)):
        got, exact = py_fma(a, b, c), Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        assert abs(Fraction(got) - exact) * 2 <= Fraction(math.ulp(got))


def _iso_fma(mu):
    mu = [float(v) for v in mu]

    def logobj(x):
        q = 0.0
        for i in range(len(mu)):
            r = x[i] - mu[i]
            q = r * r if i == 0 else py_fma(r, r, q)
        return -q
    return logobj


def _iso_two_roundings(mu):
    mu = [float(v) for v in mu]

    def logobj(x):
        q = 0.0
        for i in range(len(mu)):
            r = x[i] - mu[i]
            q = r * r if i == 0 else r * r + q
        return -q
    return logobj


def test_the_oracles_iso_sum_is_an_fma_chain(oracle):
    """The precondition of the next test: the oracle's ISO is r0*r0, then fma(r, r, q) -- and not the two-rounding sum."""
    d = 10
    mu = np.random.default_rng(1).random(d)
    X = np.random.default_rng(2).standard_normal((200, d))
    prob = oracle.Problem(200, d, 5, 400, np.ones(d), 0, target=demc.IsoQuadTarget(mu).spec())
    lp = oracle.logp(prob, X)
    fused, plain = _iso_fma(mu), _iso_two_roundings(mu)
    assert all(lp[c] == fused(X[c].tolist()) for c in range(200))
    assert any(lp[c] != plain(X[c].tolist()) for c in range(200))


def _driver_inputs(d, poisoned, tempered):
    N, K, G = 20, 5, 30
    w = demc.workloads.iso_quad_problem(d, N)
    Zinit = poisoned_population(d, N, 3) if poisoned else w["Zinit"]
    eps = np.array(w["eps_scale"])
    eps[0] = 1e-320
    T = np.array([demc.tempbaseline(g, G, 3, 1e-3) for g in range(1, G + 1)]) if tempered else None
    return w, Zinit, N, K, G, eps, T


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("poisoned", [False, True])
@pytest.mark.parametrize("d", [3, 10])
def test_python_driver_equals_the_oracle(oracle, d, poisoned, tempered):
    w, Zinit, N, K, G, eps, T = _driver_inputs(d, poisoned, tempered)
    ref = oracle_sample(oracle, w["target"], Zinit, N, K, G, None, eps, w["gamma"], 11, temperature=T)
    got = oracle_sample_logobj(oracle, _iso_fma(w["mu"]), Zinit, N, K, G, None, eps, w["gamma"], 11, temperature=T)
    same_bits(got, ref, what=f"d={d}")
    assert got["M"] == ref["M"] and np.array_equal(got["changed"], ref["changed"])
    assert np.count_nonzero(nf.chains_that_move(ref, Zinit[-N:])) >= N // 2
    if poisoned:
        with np.errstate(invalid="ignore"):
            assert not np.isfinite(ref["log_obj"]).all() and np.isnan(np.diff(ref["log_obj"], axis=1)).any()


@pytest.mark.parametrize("blocks", [[[0], [1, 2]], [[2, 0], [1]]])
def test_python_driver_equals_the_oracle_with_blocks(oracle, blocks):
    w, Zinit, N, K, G, eps, T = _driver_inputs(3, True, True)
    ref = oracle_sample(oracle, w["target"], Zinit, N, K, G, blocks, eps, w["gamma"], 11, temperature=T)
    got = oracle_sample_logobj(oracle, _iso_fma(w["mu"]), Zinit, N, K, G, blocks, eps, w["gamma"], 11, temperature=T)
    same_bits(got, ref)
    assert np.array_equal(got["changed"], ref["changed"])


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("poisoned", [False, True])
@pytest.mark.parametrize("d", [3, 10])
def test_infinite_box_is_the_plain_quadratic(oracle, d, poisoned, tempered):
    """BOX's twin with h = inf: no candidate violates it, a NaN residual comes out as a NaN sum -- the two-rounding quadratic,
    bit for bit (the oracle's own ISO is an fma chain: equal to it only where no rounding differs, which is not asserted)."""
    w, Zinit, N, K, G, eps, T = _driver_inputs(d, poisoned, tempered)
    a = oracle_sample_logobj(oracle, box_closure(w["mu"], np.full(d, np.inf)), Zinit, N, K, G, None, eps, w["gamma"], 11, temperature=T)
    b = oracle_sample_logobj(oracle, _iso_two_roundings(w["mu"]), Zinit, N, K, G, None, eps, w["gamma"], 11, temperature=T)
    same_bits(a, b)
    assert np.array_equal(a["changed"], b["changed"])


# ---- conditions on the reference, row by row -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nf.BUILTIN_ROWS)
def test_reference_run_of_each_row_has_what_the_gpu_test_needs(oracle, case):
    r = nf.row_inputs(case)
    ref = nf.reference(oracle, r)
    N = r["N"]
    X0 = r["Zinit"][-N:]
    lp0 = oracle.logp(ref["prob"], X0)
    lp_hist = np.concatenate([lp0[:, None], ref["log_obj"]], axis=1)
    moved = np.count_nonzero(nf.chains_that_move(ref, X0))
    never_finite = np.count_nonzero(~np.isfinite(lp_hist).any(axis=1))
    with np.errstate(invalid="ignore"):
        nan_events = np.count_nonzero(np.isnan(np.diff(lp_hist, axis=1)))
        assert np.array_equal(ref["changed"], (np.diff(lp_hist, axis=1) != 0).sum(axis=0))
    bad_rows = np.count_nonzero(~np.isfinite(ref["Z"]).all(axis=1))
    print(f"{case}: {moved}/{N} chains move, {never_finite} never finite, {nan_events} NaN-difference events, {bad_rows} non-finite archive rows")
    assert 2 * moved >= N                                  # (a)
    assert never_finite >= 1                               # (b)
    assert nan_events >= 1                                 # (c)
    assert bad_rows >= 1                                   # (d)


def test_negative_zero_and_subnormals_occur_in_some_chain_history(oracle):
    """Over the whole table, not per row: the rows are taken in the table's order until both have been seen."""
    negative_zero = subnormal = 0
    for case in nf.BUILTIN_ROWS:
        ch = nf.reference(oracle, nf.row_inputs(case))["chain"]
        negative_zero += np.count_nonzero(ch.view(np.uint64) == np.uint64(0x8000000000000000))
        subnormal += np.count_nonzero((np.abs(ch) > 0) & (np.abs(ch) < TINY))
        if negative_zero and subnormal:
            break
    assert negative_zero > 0 and subnormal > 0, (negative_zero, subnormal)


# ---- subnormal worlds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,case,tempered", nf.WORLD_CASES)
def test_subnormal_worlds_are_subnormal(oracle, world, case, tempered):
    r = nf.world_inputs(world, case, tempered)
    ref = nf.reference(oracle, r)
    N = r["N"]
    moved = np.count_nonzero(nf.chains_that_move(ref, r["Zinit"][-N:]))
    share = nf.subnormal_share(ref["log_obj"])
    print(f"{world} {case} tempered={tempered}: subnormal share of log_obj {share:.3f}, {len(np.unique(ref['log_obj']))} distinct of "
          f"{ref['log_obj'].size}, {moved}/{N} chains move, subnormal share of chain {nf.subnormal_share(ref['chain']):.3f}")
    if world == "mvn":
        assert 2 * moved >= N
        assert nf.subnormal_share(ref["chain"]) >= 0.9 and len(np.unique(ref["log_obj"])) == 1
        assert not ref["changed"].any()                    # every proposal accepted, no log_obj changed: the count is of differences
    else:
        assert share >= 0.9
        assert 2 * moved >= N


# ---- program cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,N,tempered", [c for c in nf.PROGRAM_GRID if c[2] == 64])
def test_program_cases_hold_what_they_are_for(oracle, name, d, N, tempered):
    """The conditions test_gpu_nonfinite.py puts on the reference of its program cases, at the smaller population (the twins run
    here: no exception where IEEE has a value)."""
    r = nf.program_inputs(name, d, N, tempered)
    facts = nf.program_reference_facts(r, nf.program_reference(oracle, r))
    assert 2 * facts["moved"] >= N, facts
    if name in ("box", "sqrtdom"):
        assert 0.15 * N <= facts["outside_at_start"] <= 0.4 * N and facts["finite_chain_rejected_outside"] >= 1, facts
    if name in ("box", "box_poisoned"):
        assert facts["entered"] >= 1, facts
    if name == "sqrtdom":
        assert facts["entered"] == 0, facts                 # NaN outside the support: every difference rejects
    if name == "pole":
        assert facts["captured"] >= 1 and 2 * facts["captured"] <= N and facts["captured"] > facts["captured_at_start"], facts
