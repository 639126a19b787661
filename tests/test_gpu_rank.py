"""GPU: the rank kernels (K10, demcz_kernels_rank.h) and the calls around them against the NumPy reference of rank_reference.py.
Raw ranks are compared exactly, normal scores as uint64 against the restatement applied to those ranks, indicators exactly; R-hat,
ESS and quantiles of the ranked history against the extended-precision references fed the restated scores, at the tolerances of
test_gpu_stats.py and test_gpu_ess.py.  test_rank_reference.py shows without a GPU that the worlds of rank_cases.py reach the cases
they are for."""
import functools

import numpy as np
import pytest

import derive_cases as dc
import ess_reference as E
import quantile_cases as Q
import rank_cases as K
import rank_reference as RR
import stats_cases as S
import stats_reference as SR

pytestmark = pytest.mark.gpu

WORLDS = {
    "all_equal": K.all_equal, "low_byte": K.low_byte, "sign_only": K.sign_only, "high_byte_only": K.high_byte_only,
    "specials": K.specials, "lattice": K.lattice,
}


def chain_of(w):
    return S.world(*w) if isinstance(w, tuple) else WORLDS[w]()


@functools.lru_cache(maxsize=None)
def reference(w, folded=False):
    """(ranks, z) of a world, computed once; folded: at the world's type-7 median (the lattice: at its own centre)."""
    chain = chain_of(w)
    center = None
    if folded:
        center = K.LATTICE_CENTER if w == "lattice" else Q.reference(chain, (0.5,)).q[:, 0]
    r = RR.ranks_of_chain(chain, center)
    return r, RR.z_of_ranks(r), center


def same_bits(a, b):
    return np.array_equal(RR.bits(a), RR.bits(b))


def get(h):
    with h:
        return h.get()


def hold_ranking(demc, chain, r, z, center, what):
    got_r = get(demc.rank_normalize_chain(chain, center=center, ranks=True))
    bad = np.argwhere(~((got_r == r) | (np.isnan(got_r) & np.isnan(r))))
    if bad.size:
        c, p, g = bad[0]
        print(f"[rank] {what}: {len(bad)} ranks differ, first at (chain {c}, parameter {p}, generation {g}): {got_r[c, p, g]!r} vs {r[c, p, g]!r}")
    assert np.array_equal(got_r, r, equal_nan=True), what
    got_z = get(demc.rank_normalize_chain(chain, center=center))
    assert np.array_equal(np.isnan(got_z), np.isnan(z)) and same_bits(got_z[~np.isnan(z)], z[~np.isnan(z)]), what


# ---- the array form on every world ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("folded", [False, True], ids=["bulk", "folded"])
@pytest.mark.parametrize("w", K.ARRAY_WORLDS + list(WORLDS), ids=K.ids)
def test_ranks_and_scores_on_the_worlds(demc, w, folded):
    r, z, center = reference(w, folded)
    hold_ranking(demc, chain_of(w), r, z, center, f"{K.ids(w)} {'folded' if folded else 'bulk'}")


def test_all_equal_values_sit_at_the_centre(demc):
    chain = K.all_equal()
    N, _, G = chain.shape
    with demc.rank_normalize_chain(chain, ranks=True) as h:
        assert (h.get()[:, 0] == (N * G + 1) / 2).all()
    with demc.rank_normalize_chain(chain) as h:
        z = h.get()
        assert (z[:, 0] == 0.0).all() and not np.signbit(z[:, 0]).any()
        rhat = h.rhat(1, G)
        assert np.isnan(rhat[0]) and np.isfinite(rhat[1])                # 0 / 0 by the IEEE rule of demcz_rhat


@pytest.mark.parametrize("negative", [False, True], ids=["+nan", "-nan"])
def test_a_nan_spoils_its_own_parameter_only(demc, negative):
    bad, clean = K.with_nan(negative), K.without_nan()
    for ranks in (True, False):
        a = get(demc.rank_normalize_chain(bad, ranks=ranks))
        b = get(demc.rank_normalize_chain(clean, ranks=ranks))
        assert np.isnan(a[:, 1]).all() and same_bits(a[:, [0, 2]], b[:, [0, 2]]) and not np.isnan(b).any()
    med = Q.reference(clean, (0.5,)).q[:, 0]
    a = get(demc.rank_normalize_chain(bad, center=med))
    b = get(demc.rank_normalize_chain(clean, center=med))
    assert np.isnan(a[:, 1]).all() and same_bits(a[:, [0, 2]], b[:, [0, 2]])
    d = demc.rank_diagnostics_chain(bad)
    dclean = demc.rank_diagnostics_chain(clean)
    for x, y in zip(d, dclean):
        assert np.isnan(x[1]) and same_bits(x[[0, 2]], y[[0, 2]]) and np.isfinite(y).all()


# ---- statistics of the ranked history ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [(67, 2, 301), (1024, 1, 257)], ids=K.ids)
def test_statistics_of_the_ranked_history(demc, w):
    from test_gpu_ess import hold_ess, hold_undecided
    from test_gpu_quantiles import hold as hold_quantiles
    chain = chain_of(w)
    G = w[2]
    _, z, _ = reference(w)
    with demc.rank_normalize_chain(chain) as h:
        err = SR.rhat_error(h.rhat(1, G), SR.rhat_gelman(z))
        print(f"[rank] {K.ids(w)}: rhat of the scores {err:.3e}")
        assert err <= SR.RHAT_RTOL
        ref = E.ess(z)
        got, keep = h.ess(1, G), ref.margin >= E.MARGIN
        assert np.array_equal(got.ess, E.ess_of_tau(got.tau, ref.m * ref.n))
        if keep.any():
            hold_ess(got, ref, f"scores of {K.ids(w)}", keep=keep)
        else:                                                           # (every stopping pair of the reference is within MARGIN of zero)
            for p in range(len(keep)):
                hold_undecided(got, ref, p, f"scores of {K.ids(w)}")
        hold_quantiles(h.quantiles(1, G, Q.PROBS, with_order_stats=True), Q.reference(z), f"scores of {K.ids(w)}")


# ---- the indicator kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [(5, 3, 7), (67, 2, 301), "specials"], ids=K.ids)
def test_indicator_le_is_exact(demc, w):
    chain = chain_of(w)
    N, d, G = chain.shape
    q = Q.reference(chain, (0.05, 0.5, 0.95)).q
    for thr in (q, q[:, :1], np.stack([chain[0, :, 0], np.full(d, np.inf), np.full(d, -np.inf), np.zeros(d), np.full(d, np.nan)], axis=1)):
        e = _array_handle(demc, chain)
        with e.indicator_le(1, G, thr) as h:
            got = h.get()
        e.close()
        want = RR.indicator_le(chain, thr)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), K.ids(w)
    bad = K.with_nan()
    e = _array_handle(demc, bad)
    with e.indicator_le(1, bad.shape[2], Q.reference(K.without_nan(), (0.5,)).q) as h:
        got = h.get()
    e.close()
    assert np.isnan(got).sum() == 1 and np.isnan(got[33, 1, 5]) and np.array_equal(got, RR.indicator_le(bad, Q.reference(K.without_nan(), (0.5,)).q), equal_nan=True)


def _array_handle(demc, chain):
    """A handle that holds `chain` as its history: the identity program of derive_chain."""
    d = chain.shape[1]
    src = "__device__ void demcz_derive(const double* x, double, const double*, int64_t, double* out)\n" \
          "{\n    for (int k = 0; k < DEMCZ_D; ++k) out[k] = x[k];\n}\n"
    h = demc.derive_chain(chain, None, demc.DerivedProgram(src, d=d, m=d))
    assert np.array_equal(RR.bits(h.get()), RR.bits(chain))
    return h


# ---- the handle forms: a real run, windows, a derived source -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(demc):
    """The run world: IsoQuadTarget d = 3, N = 64, 200 generations at a gamma that rejects most proposals."""
    a = K.RUN
    w = demc.workloads.iso_quad_problem(a["d"], a["N"])
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=a["N"], d=a["d"], K=a["K"], Mcap=M0 + a["N"] * (a["G"] // a["K"] + 1), Gcap=a["G"], blockindex=[range(a["d"])],
                       eps_scale=w["eps_scale"], seed=a["seed"], target=w["target"])
    e.set_state(w["Zinit"][-a["N"]:], None, w["Zinit"])
    e.run(1, a["G"], a["gamma"])
    yield e
    e.close()


@pytest.mark.parametrize("window", [(1, 200), (37, 161), (2, 8)], ids=K.ids)
def test_a_real_run_full_of_ties(demc, run, window):
    a, b = window
    chain, lo = run.get_history(a, b)
    if window == (1, 200):
        assert (chain[:, :, 1:] == chain[:, :, :-1]).mean() > 0.7 and (np.diff(lo, axis=1) != 0).mean() < 0.3
    r = RR.ranks_of_chain(chain)
    z = RR.z_of_ranks(r)
    with run.rank_normalize(a, b, ranks=True) as h:
        assert (h.g_from, h.g_to) == (a, b) and np.array_equal(h.get(), r)
    with run.rank_normalize(a, b) as h:
        got = h.get()
        assert same_bits(got, z)
        assert same_bits(get(demc.rank_normalize_chain(chain)), got)                   # the array form: the same bits
        if b - a + 1 >= 100:
            assert SR.rhat_error(h.rhat(a, b), SR.rhat_gelman(z)) <= SR.RHAT_RTOL
            inner = SR.rhat_gelman(z[:, :, 10:b - a + 1 - 9])                              # a window inside the ranked history
            assert SR.rhat_error(h.rhat(a + 10, b - 9), inner) <= SR.RHAT_RTOL
    med = run.quantiles(a, b, [0.5])[:, 0]
    assert np.array_equal(med, Q.reference(chain, (0.5,)).q[:, 0])
    rf = RR.ranks_of_chain(chain, med)                                                 # a centre that equals some draws exactly
    assert (chain == med[None, :, None]).any()
    with run.rank_normalize(a, b, center=med) as h:
        assert same_bits(h.get(), RR.z_of_ranks(rf))
    with run.rank_normalize(a, b, center=med, ranks=True) as h:
        assert np.array_equal(h.get(), rf)
    thr = run.quantiles(a, b, [0.05, 0.95])
    with run.indicator_le(a, b, thr) as h:
        assert np.array_equal(h.get(), RR.indicator_le(chain, thr))


def test_rank_diagnostics_is_its_composition(demc, run):
    for a, b in [(1, 200), (37, 161)]:
        d3 = run.rank_diagnostics(a, b)
        q = run.quantiles(a, b, [0.05, 0.5, 0.95])
        with run.rank_normalize(a, b) as zb, run.rank_normalize(a, b, center=q[:, 1]) as zf, \
                run.indicator_le(a, b, q[:, [0, 2]]) as ind:
            rb, rf = zb.rhat(a, b), zf.rhat(a, b)
            bulk = zb.ess(a, b).ess
            t = ind.ess(a, b).ess
        d = run.d
        assert same_bits(d3.rhat_rank, np.maximum(rb, rf)) and same_bits(d3.ess_bulk, bulk)
        assert same_bits(d3.ess_tail, np.minimum(t[:d], t[d:]))
        again = run.rank_diagnostics(a, b)                                             # two calls: identical bits
        arr = demc.rank_diagnostics_chain(run.get_history(a, b)[0])                    # the array form: identical bits
        for x, y, zz in zip(d3, again, arr):
            assert same_bits(x, y) and same_bits(x, zz)
    s = run.get_history(1, 200)[0]
    with_keys = demc.posterior_summary(s, probs=[0.5], rank_normalized=True)
    assert sorted(with_keys) == sorted(["converged", "ess", "mcse", "mean", "quantiles", "rhat", "sd", "rhat_rank", "ess_bulk", "ess_tail"])
    full = run.rank_diagnostics(1, 200)
    assert same_bits(with_keys["rhat_rank"], full.rhat_rank) and same_bits(with_keys["ess_tail"], full.ess_tail)


def test_rank_diagnostics_against_the_reference(demc):
    for chain in (K.independent_normal(), K.scale_mixture()):
        N, d, G = chain.shape
        rhat, bulk, tail, parts = RR.diagnostics(chain)
        got = demc.rank_diagnostics_chain(chain)
        print(f"[rank] diagnostics: rhat_rank {got.rhat_rank} vs {rhat}; ess_bulk {got.ess_bulk} vs {bulk}; ess_tail {got.ess_tail} vs {tail}")
        assert SR.rhat_error(got.rhat_rank, rhat) <= SR.RHAT_RTOL
        # the ESS where the reference's stopping decisions are MARGIN from flipping: tau within the tolerance of test_gpu_ess.py
        S_ = N * G
        keep = parts["bulk"].margin >= E.MARGIN
        tau_got, tau_ref = S_ / got.ess_bulk[keep], parts["bulk"].tau[keep]
        assert (np.abs(tau_got - tau_ref) <= E.TAU_ATOL_PER_LAG * (2 * parts["bulk"].pairs[keep] + 1) + 4e-16 * np.abs(tau_ref)).all()
    plain = demc.Rhat_gelman(K.scale_mixture())
    assert (plain < 1.01).all() and (got.rhat_rank > 1.1).all()                        # the case the statistic exists for


def test_a_derived_history_as_the_source(demc):
    prog, f = dc.generic_program(demc, 3, 2)
    chain, log_obj = dc.history(70, 3, 12, seed=41)
    v = f(chain, log_obj)
    r = RR.ranks_of_chain(v)
    with demc.derive_chain(chain, log_obj, prog) as src:
        with src.rank_normalize(3, 11, ranks=True) as h:
            assert np.array_equal(h.get(), RR.ranks_of_chain(v[:, :, 2:11]), equal_nan=True)
        with src.rank_normalize(1, 12) as h:
            assert same_bits(h.get(), RR.z_of_ranks(r))
            with h.rank_normalize(1, 12, ranks=True) as again:                          # ranks of scores: the same ranks
                assert np.array_equal(again.get(), r)
        d = src.rank_diagnostics(1, 12)
        arr = demc.rank_diagnostics_chain(v)
        for x, y in zip(d, arr):
            assert same_bits(x, y)
        s = src.summary(rank_normalized=True)
        assert same_bits(s["ess_bulk"], d.ess_bulk) and set(s) == set(src.summary()) | {"rhat_rank", "ess_bulk", "ess_tail"}


def test_a_one_rank_communicator_returns_the_bits_of_a_handle_without_one(demc):
    a = K.RUN
    w = demc.workloads.iso_quad_problem(a["d"], a["N"])
    out = []
    for comm in (False, True):
        M0 = w["Zinit"].shape[0]
        e = demc.HipEngine(N=a["N"], d=a["d"], K=a["K"], Mcap=M0 + a["N"] * 5, Gcap=40, blockindex=[range(a["d"])],
                           eps_scale=w["eps_scale"], seed=3, target=w["target"])
        if comm:
            e.comm_init(e.comm_unique_id(), 1, 0)
        e.set_state(w["Zinit"][-a["N"]:], None, w["Zinit"])
        e.run(1, 40, 2.38)
        out.append((get(e.rank_normalize(1, 40)), e.rank_diagnostics(5, 36)))
        e.close()
    assert same_bits(out[0][0], out[1][0])
    for x, y in zip(out[0][1], out[1][1]):
        assert same_bits(x, y)


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_errors(demc, run):
    import ctypes as C
    L, h = run._L, run._h
    out = C.c_void_p(1)
    assert L.demcz_rank_normalize(h, 1, 200, 2, None, C.byref(out)) == 1 and not out.value            # mode out of range
    out = C.c_void_p(1)
    assert L.demcz_rank_normalize(h, 1, 200, -1, None, C.byref(out)) == 1 and not out.value
    assert L.demcz_rank_normalize(h, 1, 200, 0, None, None) == 1 and L.demcz_rank_normalize(None, 1, 200, 0, None, C.byref(out)) == 1
    assert L.demcz_rank_diagnostics(h, 1, 200, None, None, None) == 1                                   # every output NULL
    assert L.demcz_indicator_le(h, 1, 200, 1, None, C.byref(out)) == 1 and L.demcz_indicator_le(h, 1, 200, 0, None, C.byref(out)) == 1
    one = np.empty(run.d)
    assert L.demcz_rank_diagnostics(h, 1, 200, None, demc._lib.ptr(one), None) == 0 and np.isfinite(one).all()      # any may be NULL
    assert same_bits(one, run.rank_diagnostics(1, 200).ess_bulk)
    codes = []
    for f in (lambda: run.rhat(100, 201), lambda: run.rank_normalize(100, 201), lambda: run.rank_diagnostics(100, 201),
              lambda: run.indicator_le(100, 201, np.zeros(run.d)), lambda: run.rank_normalize(0, 20), lambda: run.rank_normalize(20, 19)):
        with pytest.raises(demc.DemczError) as ei:
            f()
        codes.append(ei.value.code)
    assert codes == [codes[0]] * len(codes)
    with pytest.raises(demc.DemczError) as ei:
        run.rank_diagnostics(5, 7)                                                                      # w < 4
    assert ei.value.code == 1 and "4 generations" in str(ei.value)
    with run.rank_normalize(5, 7) as h3:                                                               # (ranking itself takes any window)
        assert h3.get().shape == (run.N, run.d, 3)
    with pytest.raises(demc.DemczError):
        demc.rank_diagnostics_chain(np.zeros((4, 2, 3)))
    with pytest.raises(ValueError):
        run.rank_normalize(1, 200, center=np.zeros(run.d + 1))


def test_posterior_summary_is_unchanged_by_default(demc):
    chain = S.world(64, 3, 260)
    a, b = demc.posterior_summary(chain, probs=Q.PROBS), demc.posterior_summary(chain, probs=Q.PROBS, rank_normalized=False)
    assert sorted(a) == sorted(b) == ["converged", "ess", "mcse", "mean", "quantiles", "rhat", "sd"]
    for k in a:
        assert np.array_equal(RR.bits(a[k]), RR.bits(b[k])) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k])
    assert np.array_equal(a["quantiles"], Q.world_reference((64, 3, 260)).q)
    assert sorted(demc.posterior_summary(chain)) == ["converged", "ess", "mcse", "mean", "rhat", "sd"]
