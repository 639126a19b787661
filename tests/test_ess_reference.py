"""CPU tier of the effective-sample-size tests: the extended-precision reference (ess_reference.py) against exact rational
arithmetic; the worlds of ess_cases.py against the condition that lets test_gpu_ess.py demand equal `pairs` and `converged`;
the tolerances against a float64 restatement of the device arithmetic, which must meet them with a factor of ten to spare as
written and miss them once it centres on the grand mean instead of each split chain's own; and the host finisher
demcz_ess_from_sums, which needs no device."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ess_cases as C
import ess_reference as E
import stats_cases as S
import stats_reference as R


# ---- the reference itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", ["longdouble", "mpmath"] if R.LONGDOUBLE else ["mpmath"])
def test_autocovariance_against_exact_rational_arithmetic(use):
    """A(t) of a world with offsets (parameter 1 sits at 1e6 with sd 1) is the exact rational to 1e-17 of A(0), at every lag."""
    chain = C.world(*C.FRACTION_WORLD)
    N, d, G = chain.shape
    assert abs(chain[:, 1, :].mean()) > 9e5
    n, m = G // 2, 2 * N
    B = R.backend(use)
    ref = E.ess(chain, use=use)
    assert ref.L == n - 1 == 3
    for p in range(d):
        X = [[Fraction(float(chain[c, p, g])) for g in range(G)] for c in range(N)]
        cs = [X[c][:n] for c in range(N)] + [X[c][n:2 * n] for c in range(N)]
        mean = [sum(s) / n for s in cs]
        A = [sum(sum((s[i] - a) * (s[i + t] - a) for i in range(n - t)) for s, a in zip(cs, mean)) / (m * n) for t in range(n)]
        grand = sum(mean) / m
        between = sum((a - grand) ** 2 for a in mean)
        for t in range(n):
            assert abs(B.fraction(ref.A[p, t]) - A[t]) <= Fraction(1, 10 ** 17) * A[0], (p, t)
        assert abs(B.fraction(ref.between[p]) - between) <= Fraction(1, 10 ** 17) * between
        assert abs(B.fraction(ref.varplus[p]) - (A[0] + between / (m - 1))) <= Fraction(1, 10 ** 17) * A[0]


def test_the_reference_is_the_estimator_on_a_sequence_worked_by_hand():
    """Geyer's rule on given rho: sums chosen so that W = A(0) n/(n-1) and var+ are simple.  n = 5, m = 2, between = 0:
    var+ = A(0) = 1, W = 1.25, rho_t = A(t) - 0.25."""
    n, m = 5, 2
    A = np.array([[1.0, 0.95, 0.55, 0.85, 0.15]])            # rho = 1, .7, .3, .6, -.1  ->  P = 1.7, min(.9, 1.7); lag 4 unpaired
    r = E.finish(R.backend().lift(A * m * n), R.backend().lift(np.zeros(1)), n, m)
    _, rho, tau, pairs, conv, ess, vp, margin = r
    assert np.allclose(R.to_float(rho), [[1.0, 0.7, 0.3, 0.6, -0.1]], atol=1e-15)
    assert pairs[0] == 2 and conv[0] == 0 and abs(tau[0] - (-1 + 2 * (1.7 + 0.9))) < 1e-15 and abs(ess[0] - 10 / tau[0]) < 1e-14
    assert abs(margin[0] - 0.9) < 1e-15
    A = np.array([[1.0, 0.95, 0.55, 0.85, 0.2, 0.25, 9.0, 9.0]])       # P_2 = -0.05 + 0 stops: the lags behind it are never read
    _, _, tau, pairs, conv, _, _, margin = E.finish(R.backend().lift(A * m * n), R.backend().lift(np.zeros(1)), n, m)
    assert pairs[0] == 2 and conv[0] == 1 and abs(tau[0] - 4.2) < 1e-15 and abs(margin[0] - 0.05) < 1e-15
    A = np.array([[1.0, 0.3, 0.7, 0.9]])                      # rho = 1, .05, .45, .65: P = 1.05, 1.1 -> min = 1.05
    _, _, tau, pairs, conv, _, _, _ = E.finish(R.backend().lift(A * m * n), R.backend().lift(np.zeros(1)), n, m)
    assert pairs[0] == 2 and conv[0] == 0 and abs(tau[0] - 3.2) < 1e-15


def test_the_two_number_systems_agree():
    if not R.LONGDOUBLE:
        return                                                         # (only one number system here)
    chain = C.world(65, 7, 20)
    a, b = E.ess(chain, use="mpmath"), E.ess(chain, use="longdouble")
    assert np.array_equal(a.pairs, b.pairs) and np.array_equal(a.converged, b.converged)
    assert np.allclose(a.tau, b.tau, rtol=1e-14, atol=1e-14) and np.allclose(R.to_float(a.A), R.to_float(b.A), rtol=1e-15, atol=0)
    flat = E.ess(S.all_identical(2, 2, 8), use="mpmath")
    assert np.isnan(flat.ess).all() and np.isnan(flat.tau).all() and (flat.pairs == 0).all() and (flat.converged == 1).all()


# ---- the worlds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", C.WORLDS, ids=C.ids)
def test_world_preconditions(w):
    """Every stopping decision of the reference is at least MARGIN = 1e-4 from flipping -- a hundred times what the tolerance of
    A(t) lets rho move -- so the device must return the reference's `pairs` and `converged` exactly."""
    ref = C.reference(*w)
    print(f"{w}: margin {ref.margin.min():.3e}, pairs {ref.pairs.tolist()}, converged {ref.converged.tolist()}")
    assert np.all(ref.margin >= E.MARGIN), ref.margin
    assert np.all(R.to_float(ref.varplus) > 0) and ref.L == E.lags(w[2])


def test_worlds_reach_every_branch_of_the_finisher_and_every_edge_of_the_chunk_plan():
    refs = {w: C.reference(*w) for w in C.WORLDS}
    assert refs[(65, 7, 20)].tau[3] < 0 and refs[(65, 7, 20)].ess[3] == E.ess_of_tau(-0.128, 1300) == 1300 * math.log10(1300)      # the cap
    assert refs[(1, 1, 4)].pairs[0] == 0 and refs[(1, 1, 4)].converged[0] == 1 and refs[(1, 1, 4)].tau[0] == -1.0
    assert refs[(3, 6, 2051)].pairs.max() == 82 and refs[(3, 6, 2051)].L == 1024
    assert any((r.converged == 0).any() for r in refs.values()) and any((r.converged == 1).any() for r in refs.values())
    assert any(((r.pairs >= 64) & (r.converged == 1)).any() for r in refs.values())      # a second batch of lags is needed
    # the chunk plan: one chunk shorter than a tile; a half that ends one sample before, at and one sample after a boundary
    assert C.chunk_lengths(65, 7, 20) == [10] and C.chunk_lengths(257, 6, 131) == [65] and C.chunk_lengths(64, 3, 260) == [96, 34]
    assert C.chunk_lengths(2, 2, 382) == [96, 95] and C.chunk_lengths(2, 2, 384) == [64, 64, 64] and C.chunk_lengths(2, 2, 387) == [96, 96, 1]
    big = C.chunk_lengths(3, 6, 2051)
    assert len(big) == 11 and big[0] == 96 and big[-1] == 65 and sum(big) == 1025
    assert C.chunk_lengths(1024, 5, 25000) == [1792] * 6 + [1748]                  # the flagship run: seven chunks per half
    for w in C.WORLDS:
        assert sum(C.chunk_lengths(*w)) == w[2] // 2 and min(C.chunk_lengths(*w)) >= 1


def test_odd_window_never_reads_its_last_generation():
    for w in C.WORLDS:
        if w[2] % 2:
            r = E.ess(S.with_dropped_sample_overwritten(C.world(*w)))
            assert np.array_equal(r.tau, C.reference(*w).tau)


# ---- the tolerances: a float64 restatement of the device arithmetic ----------------------------------------------------------------
def emulated(chain, own_mean=True):
    """K5's split-chain mean (x0 + sum(x - x0)/n: rounded twice), the deviations from it rounded once, products added in
    generation order, chains added pairwise (NumPy's order, not the GPU's tree), then the finisher in float64.  own_mean=False
    centres every split chain on the grand mean instead."""
    N, d, G = chain.shape
    n, m = G // 2, 2 * N
    cs = np.concatenate([chain[:, :, :n], chain[:, :, n:2 * n]], axis=0)
    x0 = cs[:, :, :1]
    mean_j = x0 + np.cumsum(cs - x0, axis=2)[:, :, -1:] / n
    grand = mean_j.sum(axis=0, keepdims=True) / m
    y = cs - (mean_j if own_mean else grand)
    L = n - 1
    sums = np.stack([np.cumsum(y[:, :, :n - t] * y[:, :, t:], axis=2)[:, :, -1].sum(axis=0) for t in range(L + 1)], axis=1)
    between = ((mean_j - grand) ** 2).sum(axis=0).ravel()
    return sums / (m * n), E.finish(sums, between, n, m)


@pytest.mark.parametrize("w", C.WORLDS, ids=C.ids)
def test_tolerances_hold_for_the_device_arithmetic_and_fail_for_the_grand_mean(w):
    ref = C.reference(*w)
    A, (_, _, tau, pairs, conv, _, vp, _) = emulated(C.world(*w))
    ea, et, ev = E.acov_error(A, ref), E.tau_error(tau, ref), E.varplus_error(vp, ref)
    print(f"{w}: A {ea:.2e}  tau {et:.2e}  var+ {ev:.2e}")
    assert ea <= 0.1 * E.ACOV_RTOL and et <= 0.1 * E.TAU_ATOL_PER_LAG and ev <= 0.1 * E.VARPLUS_RTOL
    assert np.array_equal(pairs, ref.pairs) and np.array_equal(conv, ref.converged)
    A0, _ = emulated(C.world(*w), own_mean=False)
    e0 = E.acov_error(A0, ref)
    print(f"{w}: A centred on the grand mean {e0:.2e}")
    assert not e0 <= 100 * E.ACOV_RTOL


# ---- the finisher (host code of the library) ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finisher(demc):
    demc.build()
    return demc.ess_from_sums


@pytest.mark.parametrize("w", C.WORLDS, ids=C.ids)
def test_finisher_on_the_reference_sums(finisher, w):
    """Fed the reference's sums rounded to double it returns the reference's pairs and converged, tau within 1e-12 per lag used,
    and ess = S / tau or the cap, from its own tau, exactly."""
    ref = C.reference(*w)
    got = finisher(ref.m, ref.n, R.to_float(ref.sums), R.to_float(ref.between))
    err = float(np.max(np.abs(got.tau - ref.tau) / (2 * ref.pairs + 1)))
    print(f"{w}: tau {err:.2e}")
    assert np.array_equal(got.pairs, ref.pairs) and np.array_equal(got.converged, ref.converged)
    assert err <= 1e-12
    assert np.array_equal(got.ess, E.ess_of_tau(got.tau, ref.m * ref.n))
    assert np.allclose(got.varplus, R.to_float(ref.varplus), rtol=1e-15, atol=0)
    if ref.L >= 2 and ref.L % 2 == 0:                        # nlags odd: the last, unpaired lag is ignored
        sums = R.to_float(ref.sums).copy()
        sums[:, -1] = 1e300
        again = finisher(ref.m, ref.n, sums, R.to_float(ref.between))
        assert np.array_equal(again.tau, got.tau) and np.array_equal(again.pairs, got.pairs)


def test_finisher_never_looks_past_its_stopping_pair(finisher):
    """What lets demcz_ess stop early: the lags behind the stopping pair of every parameter can hold anything."""
    ref = C.reference(3, 6, 2051)
    assert (ref.converged == 1).all()
    sums, between = R.to_float(ref.sums), R.to_float(ref.between)
    full = finisher(ref.m, ref.n, sums, between)
    cut = 2 * int(ref.pairs.max()) + 2
    short = finisher(ref.m, ref.n, sums[:, :cut], between)
    for a, b in zip(full, short):
        assert np.array_equal(a, b)
    shorter = finisher(ref.m, ref.n, sums[:, :cut - 2], between)
    assert shorter.converged[4] == 0 and shorter.pairs[4] == ref.pairs[4]


def test_finisher_edges(finisher):
    m, n = 10, 6
    S_ = m * n
    # var+ = 0 -> NaN; NaN sums -> NaN, converged = 1, pairs = 0; the other parameter is untouched
    sums = np.array([[0.0, 0.0, 0.0, 0.0], [np.nan, 1.0, 1.0, 1.0], [60.0, 30.0, -50.0, 0.0]])
    got = finisher(m, n, sums, np.array([0.0, 1.0, 0.9]))
    assert np.isnan(got.ess[:2]).all() and np.isnan(got.tau[:2]).all() and (got.pairs[:2] == 0).all() and (got.converged[:2] == 1).all()
    assert got.varplus[0] == 0.0 and np.isnan(got.varplus[1])
    assert np.isfinite(got.ess[2]) and got.pairs[2] == 1 and got.converged[2] == 1 and got.varplus[2] == 1.0 + 0.9 / 9
    # constant chains that differ from each other: A(t) = 0, var+ > 0, rho_t = 1 for every t
    got = finisher(m, n, np.zeros((1, 6)), np.array([2.0]))
    assert got.pairs[0] == 3 and got.converged[0] == 0 and got.tau[0] == 11.0 and got.ess[0] == S_ / 11.0
    # tau below 1 / log10(S), here negative: the cap; tau itself is returned uncapped
    got = finisher(m, n, np.array([[60.0, -40.0, 10.0, -50.0]]), np.array([0.0]))
    assert got.tau[0] < 1.0 / np.log10(S_) and got.ess[0] == S_ * np.log10(S_) and got.pairs[0] == 1
    # one lag only: no pair at all
    got = finisher(m, n, np.array([[60.0]]), np.array([0.0]))
    assert got.pairs[0] == 0 and got.converged[0] == 0 and got.tau[0] == -1.0 and got.ess[0] == S_ * np.log10(S_)


def test_finisher_rejects_invalid_arguments(demc):
    import ctypes as ct
    demc.build()
    lib = ct.CDLL(str(demc.LIB_PATH))
    dp, lp, ip = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int32)
    f = lib.demcz_ess_from_sums
    f.argtypes = [ct.c_int32, ct.c_int64, ct.c_int64, ct.c_int64, dp, dp, dp, dp, dp, lp, ip]
    f.restype = ct.c_int32
    sums, between, ess = (ct.c_double * 4)(4.0, 1.0, 0.5, 0.1), (ct.c_double * 1)(0.0), (ct.c_double * 1)()
    none_d, none_l, none_i = ct.cast(None, dp), ct.cast(None, lp), ct.cast(None, ip)
    assert f(1, 2, 4, 4, sums, between, ess, none_d, none_d, none_l, none_i) == 0          # only ess is required
    assert f(0, 2, 4, 4, sums, between, ess, none_d, none_d, none_l, none_i) == 1          # d <= 0
    assert f(1, 2, 1, 4, sums, between, ess, none_d, none_d, none_l, none_i) == 1          # n < 2
    assert f(1, 2, 4, 0, sums, between, ess, none_d, none_d, none_l, none_i) == 1          # nlags < 1
    assert f(1, 2, 4, 4, none_d, between, ess, none_d, none_d, none_l, none_i) == 1
    assert f(1, 2, 4, 4, sums, none_d, ess, none_d, none_d, none_l, none_i) == 1
    assert f(1, 2, 4, 4, sums, between, none_d, none_d, none_d, none_l, none_i) == 1


def test_new_symbols_are_declared_bound_and_exported(demc):
    import ctypes as ct
    import re
    demc.build()
    hdr = re.sub(r"/\*.*?\*/", "", (demc.LIB_PATH.parent.parent / "include" / "demcz.h").read_text(), flags=re.S)
    lib = ct.CDLL(str(demc.LIB_PATH))
    for name in ("demcz_autocov_sums", "demcz_autocov_sums_array", "demcz_ess_from_sums", "demcz_ess", "demcz_ess_array"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in demc.SYMBOLS and hasattr(lib, name), name
    for name in ("ess_chain", "autocov_chain", "posterior_summary"):
        assert callable(getattr(demc, name))
