"""Reference of PSIS-LOO and WAIC for the tests of demcz_loo_columns and demcz_loo, restated from the papers:
Vehtari, Gelman & Gabry 2017 (PSIS-LOO, WAIC), Vehtari, Simpson, Gelman, Yao & Gabry 2024 (tail length, khat) and Zhang & Stephens
2009 (the generalised-Pareto fit).  Nothing here is taken from another package's code.

Three restatements of one column a (the pointwise log-likelihoods of one observation over S draws):

  column_ext    in the number system of tests/stats_reference.py (long double, or mpmath): two-pass variance, every sum in the
                wide format -- the judge
  column_f64    plain float64 NumPy in the device's reduction order (demcz_kernels_loo.h): lane-strided partials over 256 lanes,
                the butterfly over 64, the four waves in order, the tiles of 1024 in order; what separates it from the device is
                the last bit of exp / log / log1p / expm1
  column_naive  float64 with the textbook shortcuts: variance from sum a^2 - (sum a)^2 / S, logsumexp without the maximum

The tolerances are ten times the largest error of column_f64 against column_ext over the worlds of tests/loo_cases.py
(tests/test_loo_reference.py measures them, prints them, and holds column_f64 to a tenth of each constant).
"""
import math

import numpy as np

import stats_reference as sr

LOG_DBL_MIN = -708.3964185322641
MIN_FIT = 5

# ---- tolerances: 10 x the measured error of column_f64 against column_ext (test_loo_reference.py prints the measurements) ---------
ELPD_TOL = 3.0e-14       # |got - ref| / max(1, |ref|) of elpd_loo           measured 2.91e-15 (world many_candidates)
LPPD_TOL = 1.3e-14       # |got - ref| / max(1, |ref|) of lppd               measured 1.22e-15 (heavy_light)
PWAIC_TOL = 3.9e-15      # |got - ref| / max(|ref|, PWAIC_FLOOR) of p_waic   measured 3.82e-16 (window)
KHAT_TOL = 6.0e-13       # |got - ref| of pareto_k                           measured 5.86e-14 (far_from_zero)
PWAIC_FLOOR = 1e-300
# column_naive on far_from_zero and floor_cut: elpd_loo and lppd are -inf (exp(-800) is 0), p_waic of the column at 1e6 is off by 100 %.

# the reference's own guards (test_loo_reference.py): twice the largest miss seen
GPD_RECOVERY_TOL = 6.7e-3    # |k - k_true| and |sigma - 1| on exact quantiles, n = 1000: largest miss 3.33e-3 (sigma at k = -0.3)
CONJUGATE_TOL = 7.5e-2       # |elpd_loo_i - exact| on the conjugate model, 20 seeds x 12 observations x 4000 draws: 3.71e-2


# ---- the wide number system ---------------------------------------------------------------------------------------------------------
class _Wide:
    """exp, log, log1p, expm1 on what stats_reference.backend() lifts to."""

    def __init__(self, use=None):
        self.B = sr.backend(use)
        self.ld = self.B.name == "longdouble"
        if not self.ld:
            import mpmath
            mpmath.mp.dps = sr.MP_DIGITS
            self.mp = mpmath

    def lift(self, a):
        return self.B.lift(a)

    def _map(self, name, a):
        if self.ld:
            with np.errstate(all="ignore"):
                return getattr(np, name)(a)
        f = getattr(self.mp, name)
        return np.frompyfunc(lambda v: f(v), 1, 1)(np.asarray(a, dtype=object))

    def exp(self, a): return self._map("exp", a)
    def log(self, a): return self._map("log", a)
    def log1p(self, a): return self._map("log1p", a)
    def expm1(self, a): return self._map("expm1", a)
    def sqrt(self, a): return self._map("sqrt", a)

    def scalar(self, v):
        return self.lift(np.array([float(v)]))[0]


def tail_cap(S, r_eff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / r_eff))), and at most S - 1."""
    return max(0, min(int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / r_eff)))), S - 1))


def candidates(n):
    return 30 + int(math.floor(math.sqrt(n)))


def quartile(n):
    return int(math.floor(n / 4.0 + 0.5))


def k_threshold(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def _tail_length(a_sorted, M):
    """(n, c as float64, floor_cut): the elements with lw > c strictly.  Where c = lw_M that is a_j < a_M, exactly."""
    lwM = a_sorted[0] - a_sorted[M]
    if lwM > LOG_DBL_MIN:
        return int(np.searchsorted(a_sorted, a_sorted[M], side="left")), lwM, False
    lw = a_sorted[0] - a_sorted
    return int(np.count_nonzero(lw[:M + 1] > LOG_DBL_MIN)), LOG_DBL_MIN, True


def _bad(a):
    return bool(np.any(~np.isfinite(a)))


_NAN_ROW = dict(elpd_loo=float("nan"), pareto_k=float("nan"), n_tail=0, lppd=float("nan"), p_waic=float("nan"), k=float("nan"),
                sigma=float("nan"))


# ---- the judge ----------------------------------------------------------------------------------------------------------------------
def gpd_fit_ext(x, W):
    """(k, sigma) of exceedances x ascending (wide numbers): Zhang & Stephens' profile posterior mean with the prior of the PSIS
    papers."""
    n = x.shape[0]
    m = candidates(n)
    xn, xq = x[n - 1], x[quartile(n) - 1]
    j = W.lift(np.arange(1, m + 1, dtype=np.float64))
    b = 1 / xn + (1 - W.sqrt(m / (j - W.scalar(0.5)))) / (3 * xq)
    kj = W.log1p(-(b[:, None] * x[None, :])).sum(axis=1) / n
    L = n * (W.log(-(b / kj)) - kj - 1)
    w = 1 / W.exp(L[None, :] - L[:, None]).sum(axis=1)
    bhat = (b * w).sum()
    k = W.log1p(-(bhat * x)).sum() / n
    return k, -k / bhat


def _finite_wide(v):
    f = float(v)
    return f == f and abs(f) != float("inf")


def column_ext(a, r_eff=1.0, use=None):
    """dict(elpd_loo, pareto_k, n_tail, lppd, p_waic, k, sigma) of one column, rounded to float64 at the end."""
    a = np.sort(np.asarray(a, dtype=np.float64).ravel() + 0.0)
    S = a.size
    if _bad(a):
        return dict(_NAN_ROW)
    W = _Wide(use)
    M = tail_cap(S, r_eff)
    n, c64, floor_cut = _tail_length(a, M)
    A = W.lift(a)
    lw = A[0] - A
    c = W.scalar(LOG_DBL_MIN) if floor_cut else lw[M]
    expc = W.exp(np.array([c], dtype=A.dtype))[0]
    khat, k, sigma = float("inf"), float("nan"), float("nan")
    if n >= MIN_FIT:
        x = (W.exp(lw[:n]) - expc)[::-1]
        kw, sw = gpd_fit_ext(x, W)
        if _finite_wide(kw):
            k, sigma = float(kw), float(sw)
            khat = float((n * kw + 5) / (n + 10))
            jj = W.lift(np.arange(n, 0, -1, dtype=np.float64))            # sorted position i is the tail's (n - i)-th smallest
            p = (jj - W.scalar(0.5)) / n
            lp = W.log1p(-p)
            q = -(sw * lp) if float(kw) == 0.0 else sw * W.expm1(-(kw * lp)) / kw
            sm = W.log(q + expc)
            lw = lw.copy()
            lw[:n] = np.where(sm < 0, sm, W.scalar(0.0))
    da = A - A[S - 1]
    elpd = A[0] + (W.log(np.array([W.exp(lw + (A - A[0])).sum()], dtype=A.dtype))[0] - W.log(np.array([W.exp(lw).sum()], dtype=A.dtype))[0])
    lppd = A[S - 1] + (W.log(np.array([W.exp(da).sum()], dtype=A.dtype))[0] - W.log(np.array([W.scalar(S)], dtype=A.dtype))[0])
    if S > 1:
        dev = (A - A[S // 2])
        dev = dev - dev.sum() / S
        pw = float((dev * dev).sum() / (S - 1))
    else:
        pw = float("nan")
    return dict(elpd_loo=float(elpd), pareto_k=khat, n_tail=n, lppd=float(lppd), p_waic=pw, k=k, sigma=sigma)


# ---- float64 in the device's order ----------------------------------------------------------------------------------------------------
def _wave_sum(v):
    """v: (..., 64) -> (...): the butterfly v[l] + v[l ^ off], off = 32 .. 1."""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    return v[..., 0]


def _block_sum(vals):
    """vals: (..., n) -> (...): loo_block_sum of lane-strided partials over 256 lanes."""
    n = vals.shape[-1]
    rows = -(-n // 256) if n else 0
    pad = np.zeros(vals.shape[:-1] + (rows * 256,))
    pad[..., :n] = vals
    pad = pad.reshape(vals.shape[:-1] + (rows, 256))
    lanes = np.zeros(vals.shape[:-1] + (256,))
    for r in range(rows):
        lanes = lanes + pad[..., r, :]
    w = _wave_sum(lanes.reshape(vals.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _tile_sum(vals):
    """vals: (S,) -> scalar: per tile of 1024 the lane's four elements in order, the block sum, then the tiles in order."""
    S = vals.size
    ntiles = -(-S // 1024)
    pad = np.zeros(ntiles * 1024)
    pad[:S] = vals
    pad = pad.reshape(ntiles, 4, 256)
    lanes = np.zeros((ntiles, 256))
    for k in range(4):
        lanes = lanes + pad[:, k, :]
    w = _wave_sum(lanes.reshape(ntiles, 4, 64))
    tiles = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s = 0.0
    for t in tiles:
        s = s + t
    return s


def gpd_fit_f64(x):
    """(k, sigma, khat) of exceedances x ascending, float64, psis_fit_kernel's order."""
    n = x.size
    m = candidates(n)
    xn, xq = x[n - 1], x[quartile(n) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        b = 1.0 / xn + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xq)
        kj = _block_sum(np.log1p(-(b[:, None] * x[None, :]))) / n
        L = n * ((np.log(-(b / kj)) - kj) - 1.0)
        s = np.zeros(m)
        for l in range(m):
            s = s + np.exp(L[l] - L)
        w = 1.0 / s
        bhat = 0.0
        for jj in range(m):
            bhat = bhat + b[jj] * w[jj]
        k = _block_sum(np.log1p(-(bhat * x))) / n
        return float(k), float(-(k / bhat)), float((n * k + 5.0) / (n + 10.0))


def _column_f64(a, r_eff, naive):
    a = np.sort(np.asarray(a, dtype=np.float64).ravel() + 0.0)
    S = a.size
    if _bad(a):
        return dict(_NAN_ROW)
    M = tail_cap(S, r_eff)
    n, c, _ = _tail_length(a, M)
    a0, amax, shift = a[0], a[S - 1], a[S // 2]
    expc = math.exp(c)
    lw = a0 - a
    khat, k, sigma = float("inf"), float("nan"), float("nan")
    with np.errstate(all="ignore"):
        if n >= MIN_FIT:
            x = (np.exp(a0 - a[:n]) - expc)[::-1]
            kk, ss, kh = gpd_fit_f64(np.ascontiguousarray(x))
            if math.isfinite(kk):
                k, sigma, khat = kk, ss, kh
                jj = np.arange(n, 0, -1, dtype=np.float64)
                p = (jj - 0.5) / n
                lp = np.log1p(-p)
                q = -(sigma * lp) if k == 0.0 else (sigma * np.expm1(-(k * lp))) / k
                v = np.log(q + expc)
                lw = lw.copy()
                lw[:n] = np.where(v < 0.0, v, 0.0)
        if naive:
            elpd = math.log(np.exp(lw + a).sum()) - math.log(np.exp(lw).sum()) if np.exp(lw + a).sum() > 0 else float("-inf")
            se = np.exp(a).sum()
            lppd = (math.log(se) if se > 0 else float("-inf")) - math.log(S)
            pw = float((np.sum(a * a) - np.sum(a) ** 2 / S) / (S - 1)) if S > 1 else float("nan")
        else:
            d0, da, dv = a - a0, a - amax, a - shift
            s0, s1, s2 = _tile_sum(np.exp(lw)), _tile_sum(np.exp(lw + d0)), _tile_sum(np.exp(da))
            s3, s4 = _tile_sum(dv), _tile_sum(dv * dv)
            elpd = a0 + (math.log(s1) - math.log(s0))
            lppd = amax + (math.log(s2) - math.log(float(S)))
            if S > 1:
                pw = (s4 - (s3 * s3) / float(S)) / (float(S) - 1.0)
                pw = pw if pw > 0.0 else 0.0
            else:
                pw = float("nan")
    return dict(elpd_loo=float(elpd), pareto_k=khat, n_tail=n, lppd=float(lppd), p_waic=float(pw), k=k, sigma=sigma)


def column_f64(a, r_eff=1.0):
    return _column_f64(a, r_eff, naive=False)


def column_naive(a, r_eff=1.0):
    return _column_f64(a, r_eff, naive=True)


# ---- arrays and records -------------------------------------------------------------------------------------------------------------
FIELDS = ("elpd_loo", "pareto_k", "n_tail", "lppd", "p_waic")


def columns(loglik, r_eff=None, how=column_ext):
    """loglik: N x nobs x w.  dict of arrays of nobs per field of FIELDS (and k, sigma)."""
    loglik = np.asarray(loglik, dtype=np.float64)
    nobs = loglik.shape[1]
    r = np.broadcast_to(np.asarray(1.0 if r_eff is None else r_eff, dtype=np.float64), (nobs,))
    rows = [how(loglik[:, p, :], float(r[p])) for p in range(nobs)]
    out = {f: np.array([row[f] for row in rows], dtype=np.float64) for f in FIELDS + ("k", "sigma")}
    out["n_tail"] = out["n_tail"].astype(np.int64)
    return out


def errors(got, ref):
    """The four error figures the tolerances bound, each the largest over the columns where the reference is finite; a column
    whose reference is NaN or infinite must agree exactly (returned as the count of such mismatches)."""
    out, mismatch = {}, 0
    scales = dict(elpd_loo=lambda r: np.maximum(1.0, np.abs(r)), lppd=lambda r: np.maximum(1.0, np.abs(r)),
                  p_waic=lambda r: np.maximum(np.abs(r), PWAIC_FLOOR), pareto_k=lambda r: np.ones_like(r))
    for f, scale in scales.items():
        g, r = np.asarray(got[f], dtype=np.float64), np.asarray(ref[f], dtype=np.float64)
        fin = np.isfinite(r)
        mismatch += int(np.count_nonzero(~((g[~fin] == r[~fin]) | (np.isnan(g[~fin]) & np.isnan(r[~fin])))))
        with np.errstate(all="ignore"):
            e = np.abs(g[fin] - r[fin]) / scale(r[fin])
        e = np.where(np.isnan(e), np.inf, e)
        out[f] = float(e.max()) if e.size else 0.0
    return out, mismatch


TOLERANCES = lambda: dict(elpd_loo=ELPD_TOL, lppd=LPPD_TOL, p_waic=PWAIC_TOL, pareto_k=KHAT_TOL)      # noqa: E731


def record_totals(cols, S):
    """The totals and standard errors of a LOO record, NumPy on the per-observation arrays."""
    e, l, w = cols["elpd_loo"], cols["lppd"], cols["p_waic"]
    nobs = e.size
    p_loo_i, elpd_waic_i = l - e, l - w
    se = lambda v: float(np.sqrt(nobs * np.var(v, ddof=1))) if nobs > 1 else float("nan")     # noqa: E731
    return dict(elpd_loo=float(e.sum()), p_loo=float(p_loo_i.sum()), elpd_waic=float(elpd_waic_i.sum()), p_waic=float(w.sum()),
                se_elpd_loo=se(e), se_elpd_waic=se(elpd_waic_i), k_threshold=k_threshold(S),
                bad_k=np.flatnonzero(cols["pareto_k"] > k_threshold(S)))
