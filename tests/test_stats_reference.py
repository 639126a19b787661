"""CPU tier of the statistics tests: the extended-precision reference (stats_reference.py) against exact rational arithmetic and
against the oracle; the worlds of stats_cases.py against the conditions the GPU tests rely on; and the tolerances against a float64
emulation of the device algorithm, which must meet them with room to spare as written and miss them by far once its shift by a
first sample is taken out -- so a kernel that lost the shift cannot pass test_gpu_stats.py."""
from fractions import Fraction

import numpy as np
import pytest

import stats_cases as S
import stats_reference as R

WORLDS = S.all_worlds()
ids = lambda w: "x".join(str(v) for v in w)      # noqa: E731


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_long_double_is_wider_than_double_or_mpmath_is_there():
    if R.LONGDOUBLE:
        assert np.finfo(np.longdouble).eps < 2e-19 and R.backend().name == "longdouble"
    else:
        import mpmath                                                  # noqa: F401
        assert R.backend().name == "mpmath"


def _exact_rhat2_mean_cov(chain):
    """utils.jl:2-20 and :96-111 in fractions.Fraction: no rounding anywhere."""
    N, d, G = chain.shape
    X = [[[Fraction(float(chain[c, p, g])) for g in range(G)] for p in range(d)] for c in range(N)]
    n, m = G // 2, 2 * N
    rhat2 = []
    for p in range(d):
        cs = [X[c][p][:n] for c in range(N)] + [X[c][p][n:2 * n] for c in range(N)]
        avg_chains = [sum(s) / n for s in cs]
        avg_par = sum(sum(s) for s in cs) / (m * n)
        B = Fraction(n, m - 1) * sum((a - avg_par) ** 2 for a in avg_chains)
        sj = [Fraction(1, n - 1) * sum((v - a) ** 2 for v in s) for s, a in zip(cs, avg_chains)]
        W = Fraction(1, m) * sum(sj)
        varhat = Fraction(n - 1, n) * W + Fraction(1, n) * B
        rhat2.append(varhat / W)
    b = [sum(X[c][p][g] for c in range(N) for g in range(G)) / (N * G) for p in range(d)]
    cov = [[sum((X[c][p][g] - b[p]) * (X[c][q][g] - b[q]) for c in range(N) for g in range(G)) / (N * G) for q in range(d)]
           for p in range(d)]
    return rhat2, b, cov


@pytest.mark.parametrize("use", ["longdouble", "mpmath"] if R.LONGDOUBLE else ["mpmath"])
def test_reference_against_exact_rational_arithmetic(use):
    """On a world with offsets (parameter 1 sits at 1e6 with sd 1) the reference's R-hat squared (no root to argue about), mean
    and covariance are the exact rationals to 1e-17 relative: eight digits more than the tightest device tolerance."""
    chain = S.world(*S.FRACTION_WORLD)
    d = chain.shape[1]
    assert abs(chain[:, 1, :].mean()) > 9e5
    rhat2, b, cov = _exact_rhat2_mean_cov(chain)
    B = R.backend(use)
    got = R.rhat_parts(chain, use)["rhat2"]
    gb, gc = R.mean_cov_ext(chain, use)
    for p in range(d):
        assert abs(B.fraction(got[p]) - rhat2[p]) <= Fraction(1, 10 ** 17) * rhat2[p]
        assert abs(B.fraction(gb[p]) - b[p]) <= Fraction(1, 10 ** 17) * abs(b[p])
        for q in range(d):
            scale2 = cov[p][p] * cov[q][q]
            assert (B.fraction(gc[p, q]) - cov[p][q]) ** 2 <= Fraction(1, 10 ** 34) * scale2


def test_the_two_number_systems_agree():
    """The mpmath evaluation (the fall-back where long double is a double) gives the long double one's float64 results."""
    if not R.LONGDOUBLE:
        return                                                         # (only one number system here)
    chain = S.world(3, 33, 65)[:, :7, :21]
    assert np.allclose(R.rhat_gelman(chain, "mpmath"), R.rhat_gelman(chain, "longdouble"), rtol=4e-16, atol=0)
    for a, b in zip(R.mean_cov_chain(chain, "mpmath"), R.mean_cov_chain(chain, "longdouble")):
        assert np.allclose(a, b, rtol=1e-15, atol=0)
    flat = S.all_identical(2, 2, 4)
    assert np.isnan(R.rhat_gelman(flat, "mpmath")).all() and np.isposinf(R.rhat_gelman(S.constant_in_time(2, 2, 4), "mpmath")).all()


@pytest.mark.parametrize("w", [(257, 20, 131), (3, 33, 65), (600, 9, 20), (1, 5, 4), (257, 64, 40)], ids=ids)
def test_reference_against_the_oracle_on_benign_data(oracle, w):
    """The existing pin, kept: with every offset 0 the oracle's float64 loops are good to 1e-12, and the reference agrees."""
    chain = S.world(*w, offsets=False)
    assert np.allclose(oracle.rhat_gelman(chain), S.rhat_reference(*w, offsets=False), rtol=1e-12, atol=0)
    om, oc = oracle.mean_cov_chain(chain)
    rm, rc = S.meancov_reference(*w, offsets=False)
    assert R.mean_error(om, rm, rc) <= 1e-12 and R.cov_error(oc, rc) <= 1e-12


@pytest.mark.parametrize("N,G", S.ACCEPT_SHAPES)
def test_accept_reference_is_the_oracle_count(oracle, N, G):
    los = [S.logobj_random(N, G), S.logobj_on_chunk_boundaries(N, G, 0), S.logobj_on_chunk_boundaries(N, G, 1)]
    for lo in los:
        assert np.array_equal(R.changed_per_chain(lo), oracle.changed_per_chain(lo))
    r = R.accept_ratio(los[0])
    assert r[0] == (1.0 if N > 1 else r[0]) and r[-1] == (0.0 if N > 1 else r[-1])
    if N >= 63:
        assert len(np.unique(r)) > min(G - 1, N) // 3                   # (p_c really runs from 0 to 1)
    per = S.accept_chunk_length(N, G)
    for phase, lo in ((0, los[1]), (1, los[2])):
        expect = len([t for t in range(1, G) if t % per == phase % per])
        assert expect >= 1 and np.array_equal(R.changed_per_chain(lo), np.full(N, expect))


def test_shapes_reach_the_chunking_edges_they_are_for():
    """Accept ratio: w = 32770 with few chains is 1024 chunks of 33 differences, the last of them empty.  Mean / covariance:
    8200 generations of three chains are 512 chunks of 17, the last 29 empty.  R-hat: halves of 65 samples are chunks of 33 and 32
    (neither a multiple of the eight-way unrolled loop), halves of 1025 are 32 chunks with a last one of 2."""
    assert S.accept_chunk_length(3, 32770) == 33 and 1024 * 33 - 32769 >= 33
    assert (S.accept_chunk_length(64, 34), S.accept_chunk_length(65, 1026), S.accept_chunk_length(4100, 40)) == (17, 32, 20)
    mc = S.meancov_chunk_lengths(3, 2, 8200)
    assert len(mc) == 512 and mc[0] == 17 and mc.count(0) == 29 and sum(mc) == 8200
    assert S.rhat_chunk_lengths(131) == [33, 32] and S.rhat_chunk_lengths(130) == [33, 32]
    big = S.rhat_chunk_lengths(2051)
    assert len(big) == 32 and big[0] == 33 and big[-1] == 2 and sum(big) == 1025
    assert S.rhat_chunk_lengths(4100) == [65] * 31 + [35] and S.rhat_chunk_lengths(4) == [2]


def test_uncountable_pairs(oracle):
    lo, expect = S.logobj_uncountable()
    assert np.array_equal(R.changed_per_chain(lo), expect) and np.array_equal(oracle.changed_per_chain(lo), expect)
    assert np.signbit(lo[0, 1]) and not np.signbit(lo[0, 0]) and lo[0, 1] == lo[0, 0]
    assert np.array_equal(R.accept_ratio(lo), expect / np.float64(lo.shape[1] - 1))


# ---- the worlds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WORLDS, ids=ids)
def test_world_preconditions(w):
    """W > 0 and R-hat in (0.9, 1.5) for every parameter (the per-chain constant makes it differ from 1); all d(d+1)/2 covariance
    entries differ pairwise by more than the tolerance of either, so an entry read from another tile's slot shows."""
    N, d, G = w
    chain = S.world(*w)
    off, sd = S.scales(d)
    assert np.all(np.abs(off / sd) <= 1.2e6 + 1e-6)
    if d >= 2:
        assert np.max(np.abs(chain.mean(axis=(0, 2))) / chain.std(axis=(0, 2))) > 1e5
    if S.has_rhat(w):
        parts = R.rhat_parts(chain)
        rh = S.rhat_reference(*w)
        assert np.all(R.to_float(parts["W"]) > 0)
        assert np.all((rh > 0.9) & (rh < 1.5)), rh
        assert np.max(np.abs(rh - 1.0)) > 1e-3
    if N * G > 1:
        _, cov = S.meancov_reference(*w)
        iu = np.triu_indices(d)
        v = cov[iu]
        tol = R.COV_RTOL * np.sqrt(np.outer(np.diag(cov), np.diag(cov)))[iu]
        gap = np.abs(v[:, None] - v[None, :])
        need = np.maximum(tol[:, None], tol[None, :])
        np.fill_diagonal(gap, np.inf)
        assert np.all(gap > need)


def test_odd_window_never_reads_its_last_generation(oracle):
    for w in S.RHAT_WORLDS:
        if w[2] % 2:
            poisoned = S.with_dropped_sample_overwritten(S.world(*w))
            assert np.array_equal(R.rhat_gelman(poisoned), S.rhat_reference(*w))
            assert np.array_equal(oracle.rhat_gelman(poisoned), oracle.rhat_gelman(S.world(*w)))


def test_degenerate_worlds():
    c = S.constant_in_time()
    assert np.all(np.diff(c, axis=2) == 0) and len(np.unique(c[:, 0, 0])) == c.shape[0] and c.min() > 9e5
    assert np.isposinf(R.rhat_gelman(c)).all()
    assert np.isnan(R.rhat_gelman(S.all_identical())).all()
    one = S.world(*S.MEANCOV_EXACT)
    m, cov = R.mean_cov_chain(one)
    assert np.array_equal(m, one[0, :, 0]) and np.array_equal(cov, np.zeros((3, 3)))


def test_contaminated_worlds_differ_in_one_sample():
    clean = S.world(*S.CONTAMINATED)
    for v in (np.nan, np.inf):
        bad = S.contaminated(v)
        differs = ~((bad == clean) | (np.isnan(bad) & np.isnan(clean)))
        assert differs.sum() == 1 and differs[S.POISON_AT] and S.POISON_AT[1] == 11 and S.POISON_AT != (0, 11, 0)


# ---- the tolerances: a float64 emulation of the device algorithm, with and without its shift --------------------------------------
def emulated_rhat(chain, shift):
    """K5 in NumPy float64 (NumPy's summation order, not the GPU's): per split chain S1 = sum(x - x0), S2 = sum((x - x0)^2) with
    x0 its first sample, mean_j = x0 + S1/n, s_j^2 = (S2 - S1^2/n)/(n - 1); then utils.jl:13-18."""
    N, d, G = chain.shape
    n, m = G // 2, 2 * N
    cs = np.concatenate([chain[:, :, :n], chain[:, :, n:2 * n]], axis=0)
    x0 = cs[:, :, :1] if shift else np.zeros((m, d, 1))
    v = cs - x0
    S1, S2 = v.sum(axis=2), (v * v).sum(axis=2)
    mean_j = x0[:, :, 0] + S1 / n
    s2_j = (S2 - S1 * S1 / n) / (n - 1)
    gm = mean_j.sum(axis=0) / m
    B = n / (m - 1) * ((mean_j - gm) ** 2).sum(axis=0)
    W = s2_j.sum(axis=0) / m
    with np.errstate(all="ignore"):
        return np.sqrt(((n - 1) / n * W + B / n) / W)


def emulated_mean_cov(chain, shift):
    """K7b in NumPy float64: sums of (x_p - ref_p) and of (x_p - ref_p)(x_q - ref_q) with ref = chain 0's first sample, then
    mean = ref + S/cnt and cov = S_pq/cnt - dm_p dm_q."""
    N, d, G = chain.shape
    ref = chain[0, :, 0] if shift else np.zeros(d)
    flat = (chain - ref[None, :, None]).transpose(1, 2, 0).reshape(d, G * N)
    cnt = float(N * G)
    dm = flat.sum(axis=1) / cnt
    return ref + dm, flat @ flat.T / cnt - np.outer(dm, dm)


@pytest.mark.parametrize("w", WORLDS, ids=ids)
def test_tolerances_hold_with_the_shift_and_fail_without_it(w):
    """As written the emulation stays within a tenth of every tolerance on every world.  Without the shift it misses the R-hat
    and covariance tolerances by more than 100x wherever a parameter has an offset (d >= 2: parameter 1 sits at 1e6 sd)."""
    N, d, G = w
    chain = S.world(*w)
    if S.has_rhat(w):
        ref = S.rhat_reference(*w)
        e_shift, e_plain = R.rhat_error(emulated_rhat(chain, True), ref), R.rhat_error(emulated_rhat(chain, False), ref)
        print(f"rhat {w}: shifted {e_shift:.2e}, unshifted {e_plain:.2e}")
        assert e_shift <= 0.1 * R.RHAT_RTOL
        if d >= 2:
            assert not e_plain <= 100 * R.RHAT_RTOL
    rm, rc = S.meancov_reference(*w)
    (m1, c1), (m0, c0) = emulated_mean_cov(chain, True), emulated_mean_cov(chain, False)
    em, ec, ec0 = R.mean_error(m1, rm, rc), R.cov_error(c1, rc), R.cov_error(c0, rc)
    print(f"mean/cov {w}: mean {em:.2e}, cov shifted {ec:.2e}, unshifted {ec0:.2e}")
    assert em <= 0.1 * R.MEAN_RTOL and ec <= 0.1 * R.COV_RTOL
    if d >= 2:
        assert not ec0 <= 100 * R.COV_RTOL
