"""The reference of PSIS-LOO and WAIC (tests/loo_reference.py) and its tolerances, without a GPU.

  * the tolerances are ten times the largest error of the float64 restatement in the device's order against the wide reference
    over the worlds of tests/loo_cases.py; the restatement is held to a tenth of each, the naive restatement is outside;
  * the reference recovers k and sigma from exact generalised-Pareto quantiles, and agrees with the closed-form leave-one-out
    density of a conjugate normal-mean model;
  * the record's totals and loo_compare are NumPy's; the exports are in the header, in SYMBOLS and in the library;
  * PointwiseProgram.check compiles without a device and refuses what it must."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import loo_cases as lc
import loo_reference as lr

ROOT = Path(__file__).resolve().parent.parent
NEW = ["demcz_pointwise_check", "demcz_pointwise", "demcz_pointwise_array", "demcz_psis_tail_length", "demcz_gpd_fit",
       "demcz_loo_columns", "demcz_loo_columns_array", "demcz_loo", "demcz_loo_array"]


def test_tolerances_are_ten_times_the_restatements_error():
    worst = {f: 0.0 for f in lr.TOLERANCES()}
    worst_naive = dict(worst)
    for i, w in enumerate(lc.worlds()):
        ref, f64, naive = lc.reference(i), lc.restatement(i), lc.restatement(i, True)
        assert np.array_equal(f64["n_tail"], ref["n_tail"]), w["name"]
        e, mismatch = lr.errors(f64, ref)
        assert mismatch == 0, w["name"]
        en, _ = lr.errors(naive, ref)
        print(w["name"], {k: f"{v:.2e}" for k, v in e.items()}, "naive", {k: f"{v:.2e}" for k, v in en.items()})
        for f in worst:
            worst[f] = max(worst[f], e[f])
            worst_naive[f] = max(worst_naive[f], en[f])
    print("largest error of the float64 restatement:", worst)
    for f, tol in lr.TOLERANCES().items():
        assert 10.0 * worst[f] <= tol, (f, worst[f], tol)
        assert tol <= 11.0 * worst[f], (f, worst[f], tol, "the constant is no longer ten times the measured error")
    assert worst_naive["elpd_loo"] > lr.ELPD_TOL and worst_naive["lppd"] > lr.LPPD_TOL and worst_naive["p_waic"] > lr.PWAIC_TOL


@pytest.mark.skipif(not lr.sr.LONGDOUBLE, reason="long double is no wider than double here: mpmath is the only backend")
def test_the_two_number_systems_agree():
    a = lc.window_of(lc.worlds()[1])[:, 0, :]
    ld, mp = lr.column_ext(a, use="longdouble"), lr.column_ext(a, use="mpmath")
    for f in ("elpd_loo", "lppd", "p_waic", "pareto_k"):
        assert abs(ld[f] - mp[f]) <= 4e-16 * max(1.0, abs(mp[f])), f
    assert ld["n_tail"] == mp["n_tail"] == 5


def test_reference_recovers_exact_generalised_pareto_quantiles():
    W = lr._Wide()
    worst = 0.0
    for k in (-0.3, 0.2, 0.7):
        n = 1000
        p = (np.arange(1, n + 1) - 0.5) / n
        x = ((1.0 - p) ** (-k) - 1.0) / k                       # sigma = 1
        kw, sw = lr.gpd_fit_ext(W.lift(x), W)
        khat = (n * float(kw) + 5.0) / (n + 10.0)
        assert abs((khat * (n + 10.0) - 5.0) / n - float(kw)) < 1e-15        # the shrinkage undone
        worst = max(worst, abs(float(kw) - k), abs(float(sw) - 1.0))
    print("largest miss:", worst)
    assert worst <= lr.GPD_RECOVERY_TOL


def test_reference_agrees_with_the_conjugate_models_exact_loo():
    """y_i ~ N(theta, 1), theta ~ N(0, tau^2): the posterior without y_i is normal, and so is the predictive density of y_i."""
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        nobs, tau2 = 12, 4.0
        y = rng.normal(0.5, 1.0, nobs)
        prec = nobs + 1.0 / tau2
        theta = rng.normal(y.sum() / prec, 1.0 / math.sqrt(prec), 4000)
        a = -0.5 * (y[None, :, None] - theta.reshape(40, 1, 100)) ** 2 - 0.9189385332046727
        ref = lr.columns(a)
        prec_i = nobs - 1 + 1.0 / tau2
        v = 1.0 + 1.0 / prec_i
        exact = -0.5 * (y - (y.sum() - y) / prec_i) ** 2 / v - 0.5 * np.log(2.0 * np.pi * v)
        worst = max(worst, float(np.abs(ref["elpd_loo"] - exact).max()))
        assert np.all(ref["pareto_k"] < lr.k_threshold(4000))
    print("largest miss:", worst)
    assert worst <= lr.CONJUGATE_TOL


def test_record_totals_and_compare_are_numpys(demc):
    i = [w["name"] for w in lc.worlds()].index("columns33")
    ref = lc.reference(i)
    S = 16 * 30
    rec = demc.loo_record(ref["elpd_loo"], ref["pareto_k"], ref["n_tail"], ref["lppd"], ref["p_waic"], S, names=None)
    want = lr.record_totals(ref, S)
    for f in ("elpd_loo", "p_loo", "elpd_waic", "p_waic", "se_elpd_loo", "se_elpd_waic", "k_threshold"):
        assert getattr(rec, f) == want[f], f
    assert np.array_equal(rec.bad_k, want["bad_k"])
    assert np.array_equal(rec.p_loo_i, ref["lppd"] - ref["elpd_loo"]) and np.array_equal(rec.elpd_waic_i, ref["lppd"] - ref["p_waic"])
    assert rec.k_threshold == min(1.0 - 1.0 / math.log10(S), 0.7) and demc.loo_record([0.0], [0.0], [0], [0.0], [0.0], 10 ** 6).k_threshold == 0.7
    other = demc.loo_record(ref["elpd_loo"][::-1].copy(), ref["pareto_k"], ref["n_tail"], ref["lppd"], ref["p_waic"], S)
    diff = ref["elpd_loo"] - ref["elpd_loo"][::-1]
    assert demc.loo_compare(rec, other) == (float(diff.sum()), float(np.sqrt(33 * np.var(diff, ddof=1))))
    assert demc.loo_compare(rec, rec) == (0.0, 0.0)
    with pytest.raises(ValueError):
        demc.loo_compare(rec, demc.loo_record([0.0], [0.0], [0], [0.0], [0.0], S))


def test_exports_are_in_the_header_in_symbols_and_in_the_library(demc):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "demcz.h").read_text(), flags=re.S)
    assert "demcz_loglik" not in text, "the user's prototype belongs in a comment only"
    demc.build()
    lib = ctypes.CDLL(str(demc.LIB_PATH))
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in demc.SYMBOLS and hasattr(lib, name), name


def test_host_entry_points_are_the_references(demc):
    for S, r in ((1, 1.0), (2, 1.0), (400, 1.0), (8000, 1.0), (168000, 1.0), (100, 0.25), (10000, 4.0), (2 ** 31 - 1, 1.0)):
        assert demc.psis_tail_length(S, r) == lr.tail_cap(S, r)
    for bad in ((0, 1.0), (10, 0.0), (10, -1.0), (10, math.inf), (10, math.nan)):
        with pytest.raises(demc.DemczError):
            demc.psis_tail_length(*bad)
    W = lr._Wide()
    for k in (-0.3, 0.2, 0.7):
        n = 300
        p = (np.arange(1, n + 1) - 0.5) / n
        x = 2.5 * ((1.0 - p) ** (-k) - 1.0) / k
        got = demc.gpd_fit(x)
        kw, sw = lr.gpd_fit_ext(W.lift(x), W)
        assert abs(got[0] - float(kw)) <= lr.KHAT_TOL and abs(got[1] - float(sw)) <= 2.5 * lr.KHAT_TOL
        assert got[2] == (n * got[0] + 5.0) / (n + 10.0)
    with pytest.raises(demc.DemczError):
        demc.gpd_fit([1.0, 2.0, 3.0, 4.0])


def test_pointwise_program_check_compiles_without_a_device(demc):
    prog, _ = lc.gaussian_program(demc, 3, 5)
    prog.check()
    bad = demc.PointwiseProgram("__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)\n{\n"
                                "    return x[0] + undeclared;\n}\n", 3, 5)
    with pytest.raises(demc.DemczError) as ei:
        bad.check()
    assert ei.value.code == 1 and "program:3:" in str(ei.value) and "undeclared" in str(ei.value)
    with pytest.raises(demc.DemczError) as ei:
        demc.PointwiseProgram("__device__ double loglik(const double* x) { return x[0]; }", 3, 5).check()
    assert "does not define demcz_loglik" in str(ei.value)
    for d in (0, 33):
        with pytest.raises(demc.DemczError) as ei:
            demc.PointwiseProgram(prog.source, d, 5).check()
        assert ei.value.code == 1 and "1..32" in str(ei.value)
    with pytest.raises(ValueError):
        demc.PointwiseProgram(prog.source, 3, 0)
    with pytest.raises(ValueError):
        demc.PointwiseProgram(prog.source, 3, 5, names=["a"])
