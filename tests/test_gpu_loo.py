"""GPU: PSIS-LOO and WAIC on the device (demcz_pointwise, demcz_loo_columns, demcz_loo; demcz_kernels_pointwise.h, K11
demcz_kernels_loo.h) against tests/loo_reference.py over the worlds of tests/loo_cases.py.

  * the pointwise log-likelihoods equal their NumPy twins bit for bit (the programs use +, -, * and written fma only);
  * demcz_loo_columns has the reference's tail length in every world, is exact where the reference is NaN, +inf or a constant,
    and is within loo_reference's tolerances everywhere else; the largest error is printed before it is asserted;
  * demcz_loo equals demcz_loo_columns of the concatenated chunks in every bit, through every route, twice;
  * the sort's factoring left demcz_rank_normalize as it was (tests/test_gpu_rank.py is the full check).

The refusal of a communicator with several ranks (the check demcz_rank_normalize makes, shared) needs two devices and is not run
here."""
import ctypes as C

import numpy as np
import pytest

import loo_cases as lc
import loo_reference as lr
import rank_reference as RR

pytestmark = pytest.mark.gpu

N_RUN, D_RUN, G_RUN = 70, 3, 40
ARRAYS = ("elpd_loo_i", "pareto_k", "n_tail", "lppd_i", "p_waic_i")


def same_bits(a, b):
    return np.array_equal(RR.bits(np.asarray(a, dtype=np.float64)), RR.bits(np.asarray(b, dtype=np.float64)))


def same_record(a, b):
    return (all(same_bits(getattr(a, f), getattr(b, f)) for f in ARRAYS if f != "n_tail") and np.array_equal(a.n_tail, b.n_tail)
            and same_bits([a.elpd_loo, a.p_loo, a.elpd_waic, a.p_waic, a.se_elpd_loo, a.se_elpd_waic],
                          [b.elpd_loo, b.p_loo, b.elpd_waic, b.p_waic, b.se_elpd_loo, b.se_elpd_waic]))


def get(h):
    with h:
        return h.get()


def _make_engine(demc):
    w = demc.workloads.mvnormal_problem(D_RUN, N_RUN)
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N_RUN, d=D_RUN, K=w["K"], Mcap=M0 + N_RUN * (G_RUN // w["K"] + 1), Gcap=G_RUN, blockindex=[range(D_RUN)],
                       eps_scale=w["eps_scale"], seed=11, target=w["target"])
    e.set_state(w["Zinit"][-N_RUN:], None, w["Zinit"])
    e.run(1, G_RUN, w["gamma"])
    return e


@pytest.fixture(scope="module")
def run(demc):
    e = _make_engine(demc)
    yield e
    e.close()


def chunks(nobs, width=32):
    return [(f, min(nobs, f + width)) for f in range(0, nobs, width)]


# ---- pointwise: exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobs", [1, 32, 33, 70])
def test_pointwise_is_its_twin_bit_for_bit(demc, run, nobs):
    prog, twin = lc.gaussian_program(demc, D_RUN, nobs)
    chain = run.get_history(1, G_RUN)[0]
    want = twin(chain)
    for f, t in chunks(nobs):
        with run.pointwise(prog, 1, G_RUN, f, t) as h:
            got = h.get()
            assert (h.g_from, h.g_to, h.d) == (1, G_RUN, t - f) and h.names == prog.names[f:t]
        assert got.shape == (N_RUN, t - f, G_RUN) and same_bits(got, want[:, f:t, :])
        assert same_bits(get(demc.pointwise_chain(chain, prog, f, t)), want[:, f:t, :])          # the array form: the same bits


def test_pointwise_of_some_observations_in_a_window_inside_the_history(demc, run):
    prog, twin = lc.gaussian_program(demc, D_RUN, 33)
    chain = run.get_history(1, G_RUN)[0]
    with run.pointwise(prog, 7, 33, 3, 20) as h:
        assert (h.g_from, h.g_to) == (7, 33)
        assert same_bits(h.get(), twin(chain[:, :, 6:33], 3, 20))
        assert same_bits(h.get(10, 12), twin(chain[:, :, 9:12], 3, 20))
    with run.pointwise(prog, 40, 40, 32, 33) as h:                                               # one generation, the last observation
        assert same_bits(h.get(), twin(chain[:, :, 39:40], 32, 33))


# ---- loo_columns: every world --------------------------------------------------------------------------------------------------------
IDENTITY = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
#pragma unroll
    for (int k = 0; k < DEMCZ_M; ++k) out[k] = x[k];
}
"""


def _device_columns(demc, w):
    a = w["loglik"]
    if w["window"] is None:
        return demc.loo_columns_chain(a, w["r_eff"])
    g_from, g_to = w["window"]
    nobs = a.shape[1]
    with demc.derive_chain(a, None, demc.DerivedProgram(IDENTITY, nobs, nobs)) as h:
        assert same_bits(h.get(), a)
        return h.loo_columns(g_from, g_to, w["r_eff"])


def _as_cols(rec):
    return dict(elpd_loo=rec.elpd_loo_i, pareto_k=rec.pareto_k, n_tail=rec.n_tail, lppd=rec.lppd_i, p_waic=rec.p_waic_i)


@pytest.mark.parametrize("i", range(len(lc.worlds())), ids=[w["name"] for w in lc.worlds()])
def test_loo_columns_on_every_world(demc, i):
    w = lc.worlds()[i]
    ref = lc.reference(i)
    rec = _device_columns(demc, w)
    got = _as_cols(rec)
    e, mismatch = lr.errors(got, ref)
    print(f"[loo] {w['name']}: n_tail {got['n_tail'][:4]} vs {ref['n_tail'][:4]}; errors {e}; tolerances {lr.TOLERANCES()}")
    assert np.array_equal(got["n_tail"], ref["n_tail"])
    assert mismatch == 0, "a NaN, an infinite or a constant column is not exact"
    for col, want in w["expect"].items():
        if "constant" in want:
            assert got["elpd_loo"][col] == want["constant"] == got["lppd"][col] and got["p_waic"][col] == 0.0
            assert got["pareto_k"][col] == np.inf and got["n_tail"][col] == 0
    for f, tol in lr.TOLERANCES().items():
        assert e[f] <= tol, (f, e[f], tol)
    a = lc.window_of(w)
    S = a.shape[0] * a.shape[2]
    want = lr.record_totals(got, S)
    assert rec.k_threshold == want["k_threshold"] and np.array_equal(rec.bad_k, want["bad_k"])
    if np.isfinite(ref["elpd_loo"]).all():
        assert rec.elpd_loo == want["elpd_loo"] and rec.p_waic == want["p_waic"]


def test_the_neighbours_of_a_poisoned_column_are_unaffected(demc):
    names = [w["name"] for w in lc.worlds()]
    bad = demc.loo_columns_chain(lc.worlds()[names.index("poisoned")]["loglik"])
    clean = demc.loo_columns_chain(lc.worlds()[names.index("poisoned_clean_twin")]["loglik"])
    for f in ARRAYS:
        assert same_bits(getattr(bad, f)[[0, 1, 3, 6]], getattr(clean, f)[[0, 1, 3, 6]])
        assert np.all(np.isnan(getattr(bad, f)[[2, 4, 5]])) or f == "n_tail"
    assert np.array_equal(bad.n_tail[[2, 4, 5]], [0, 0, 0])


# ---- the whole thing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobs", [33, 70])
def test_loo_is_loo_columns_of_the_concatenated_chunks(demc, run, nobs):
    prog, twin = lc.gaussian_program(demc, D_RUN, nobs)
    chain = run.get_history(1, G_RUN)[0]
    loglik = np.asfortranarray(np.concatenate([get(run.pointwise(prog, 1, G_RUN, f, t)) for f, t in chunks(nobs)], axis=1))
    assert same_bits(loglik, twin(chain))
    r_eff = np.linspace(0.4, 1.6, nobs)
    for r in (None, r_eff):
        want = demc.loo_columns_chain(loglik, r)
        got = run.loo(prog, 1, G_RUN, r)
        assert same_record(got, want) and got.names == prog.names
        assert same_record(run.loo(prog, 1, G_RUN, r), got)                                      # twice: the same bits
        assert same_record(demc.loo_chain(chain, prog, r), got)                                  # the array form
    assert not np.array_equal(want.n_tail, demc.loo_columns_chain(loglik).n_tail)                # (r_eff moved the tails)
    ref = lr.columns(loglik, r_eff)
    e, mismatch = lr.errors(_as_cols(got), ref)
    assert mismatch == 0 and np.array_equal(got.n_tail, ref["n_tail"]) and all(e[f] <= tol for f, tol in lr.TOLERANCES().items()), e
    inner = run.loo(prog, 6, 36)                                                                 # a window inside the history
    assert same_record(inner, demc.loo_columns_chain(np.asfortranarray(loglik[:, :, 5:36])))


def test_a_derived_history_takes_loo_columns(demc, run):
    prog, _ = lc.gaussian_program(demc, D_RUN, 33)
    whole = run.loo(prog, 1, G_RUN)
    with run.pointwise(prog, 1, G_RUN, 0, 32) as h:
        rec = h.loo_columns(1, G_RUN)
        assert rec.names == prog.names[:32]
        for f in ARRAYS:
            assert same_bits(getattr(rec, f), getattr(whole, f)[:32])
        part = h.loo_columns(6, 36, r_eff=0.5)
        assert same_record(part, demc.loo_columns_chain(np.asfortranarray(h.get(6, 36)), 0.5))
        ess = h.ess(1, G_RUN).ess                                                                # how an r_eff is obtained
        assert ess.shape == (32,) and np.all(ess > 0)


def test_refusals(demc, run):
    prog, _ = lc.gaussian_program(demc, D_RUN, 33)
    codes = []
    for f in (lambda: run.rhat(20, G_RUN + 1), lambda: run.loo(prog, 20, G_RUN + 1), lambda: run.loo_columns(20, G_RUN + 1),
              lambda: run.pointwise(prog, 20, G_RUN + 1, 0, 3), lambda: run.loo(prog, 0, 10), lambda: run.loo_columns(12, 11)):
        with pytest.raises(demc.DemczError) as ei:
            f()
        codes.append(ei.value.code)
    assert codes == [codes[0]] * len(codes)                                                      # the range errors are demcz_rhat's
    for bad in (0.0, -1.0, np.inf, np.nan):
        for f in (lambda: run.loo(prog, 1, G_RUN, bad), lambda: run.loo_columns(1, G_RUN, bad),
                  lambda: demc.loo_columns_chain(np.zeros((4, 2, 3)), [1.0, bad])):
            with pytest.raises(demc.DemczError) as ei:
                f()
            assert ei.value.code == 1 and "r_eff" in str(ei.value)
    L, h = run._L, run._h
    src, opts, data, ndata = prog._args()
    for mc in (0, 33):
        out = C.c_void_p(1)
        assert L.demcz_pointwise(h, 1, G_RUN, 0, mc, src, opts, data, ndata, C.byref(out)) == 1 and not out.value
        assert "1..32" in L.demcz_last_error(h).decode()
    out = C.c_void_p(1)
    assert L.demcz_pointwise(h, 1, G_RUN, -1, 1, src, opts, data, ndata, C.byref(out)) == 1 and not out.value
    assert L.demcz_pointwise(None, 1, G_RUN, 0, 1, src, opts, data, ndata, C.byref(out)) == 1
    assert L.demcz_pointwise(h, 1, G_RUN, 0, 1, src, opts, data, ndata, None) == 1
    assert L.demcz_loo_columns(None, 1, G_RUN, None, None, None, None, None, None) == 1
    assert L.demcz_loo(h, 1, G_RUN, 0, src, opts, data, ndata, None, None, None, None, None, None) == 1      # nobs < 1
    with pytest.raises(ValueError):
        run.pointwise(prog, 1, G_RUN, 5, 5)
    with pytest.raises(ValueError):
        run.loo(lc.gaussian_program(demc, D_RUN + 1, 3)[0], 1, G_RUN)
    broken = demc.PointwiseProgram("__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)\n{\n"
                                   "    return nope;\n}\n", D_RUN, 3)
    with pytest.raises(demc.DemczError) as ei:
        run.loo(broken, 1, G_RUN)
    assert ei.value.code == 1 and "program:3:" in str(ei.value)
    one = np.empty(run.d)                                                                        # any output may be NULL
    assert L.demcz_loo_columns(h, 1, G_RUN, None, None, demc._lib.ptr(one), None, None, None) == 0
    assert same_bits(one, run.loo_columns(1, G_RUN).pareto_k)


# ---- the sort --------------------------------------------------------------------------------------------------------------------------
def test_rank_normalize_is_what_it_was(demc):
    rng = np.random.default_rng(5)
    chain = np.asfortranarray(np.round(rng.normal(0.0, 1.0, (70, 3, 12)), 1))                    # ties, several tiles, three columns
    chain[:, 2, :] = 4.0                                                                         # a column that sits every pass out
    r = RR.ranks_of_chain(chain)
    assert np.array_equal(get(demc.rank_normalize_chain(chain, ranks=True)), r)
    assert same_bits(get(demc.rank_normalize_chain(chain)), RR.z_of_ranks(r))
    med = np.median(chain.transpose(1, 0, 2).reshape(3, -1), axis=1)
    assert np.array_equal(get(demc.rank_normalize_chain(chain, center=med, ranks=True)), RR.ranks_of_chain(chain, med))
