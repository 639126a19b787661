"""Reference of the marginal likelihood by bridge sampling for the tests of demcz_bridge and its layers,
restated from the papers: Meng & Wong 1996 (the optimal bridge), Gronau et al. 2017 (the iterative scheme) and
Fruehwirth-Schnatter 2004 (the error estimate).  Nothing here is taken from another package's code.

Three restatements:

  bit-exact float64   cholesky, c_g, posterior_a1, proposal: the operation sequence of the spec, every fma correctly rounded
                      (fma_exact in exact fractions, as tests/loo_cases.py has it; fma_fast, the same result from error-free
                      transformations and rounding to odd -- Boldo & Melquiond 2008 -- for the arrays too large for fractions;
                      test_bridge_reference.py holds the two equal), the normals from the oracle's Philox, dm_log and Box-Muller
  iterate_ext         the iteration and the moments in the number system of tests/stats_reference.py (long double, or mpmath),
                      variances two-pass -- the judge
  iterate_f64         plain float64 NumPy in the device's order (demcz_kernels_bridge.h): tiles of 1024, lane-strided partials, the
                      butterfly over 64 lanes, the four waves and then the tiles in order, the final moments shifted by the
                      latest means; what separates it from the device is the last bit of exp and log

The tolerances are ten times the largest error of iterate_f64 against iterate_ext over the worlds of tests/bridge_cases.py
(tests/test_bridge_cases.py measures them, prints them, and holds iterate_f64 to a tenth of each constant).

se_logml depends on ESS(f2), which is demcz_ess's and has demcz_ess's own, much wider, tolerance (tests/ess_reference.py:
TAU_ATOL_PER_LAG per lag of tau).  SE_TOL therefore holds the formula: both sides are given the same ESS.  Where the device's own
ESS enters (demcz_bridge's ess_f2), it is held to the reference ESS of the reference f2 by ess_reference's tolerance of tau.
"""
import math
from fractions import Fraction

import numpy as np

import ess_reference as er
import loo_reference as lr
import oracle_py as O

LOG_2PI = 1.8378770664093453
FMA_EXACT_MAX = 20000        # elements up to which fma() goes through fractions

# ---- tolerances: 10 x the measured error of iterate_f64 against iterate_ext (test_bridge_cases.py prints the measurements) ----------
LOGML_TOL = 1.9e-15      # |got - ref| / max(1, |ref|) of logml                      measured 1.82e-16 (world offset_minus)
MOMENT_TOL = 8.3e-12     # |got - ref| / |ref| of mean f1, var f1, mean f2, var f2   measured 8.27e-13 (offset_minus: rho - a2 at 1e4)
SE_TOL = 1.7e-13         # |got - ref| / |ref| of se_logml, both with one ESS        measured 1.65e-14 (offset_minus)
F2_TOL = 9.1e-12         # |got - ref| / ref of every entry of f2 at the final rho   measured 9.03e-13 (offset_minus)
CHOL_TOL = 5.1e-15       # |(L L^T - V)_pq| / sqrt(V_pp V_qq) of the factor          measured 5.01e-16 (d = 1, 2, 5, 7, 32)

# the reference's own guard (test_bridge_reference.py): |logml - exact| / se_logml over 20 seeds of each target, twice the largest seen
GUARD_Z = 6.8            # largest miss 3.39 standard errors (the Gaussian target at d = 32)


# ---- correctly rounded fma -----------------------------------------------------------------------------------------------------------
def fma_exact(a, b, c):
    """fma(a, b, c) elementwise, correctly rounded: a b + c in exact fractions, rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
    for i in range(fa.size):
        fo[i] = float(Fraction(float(fa[i])) * Fraction(float(fb[i])) + Fraction(float(fc[i])))
    return out


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """(p, e) with p + e = a b exactly (Dekker, Veltkamp's split; no overflow or underflow in the partial products)."""
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(a, b):
    """a + b rounded to odd: the sum where it is exact, else whichever of its two neighbours has an odd significand."""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0.0) & ((bits & 1) == 0)
    toward = np.where(e > 0.0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma_fast(a, b, c):
    """fma(a, b, c) correctly rounded, in float64 arithmetic only (Boldo & Melquiond 2008): the product exactly as uh + ul, c + uh
    exactly as th + tl, tl + ul rounded to odd, and one last rounding to nearest.  For finite operands away from overflow and
    underflow -- which is where the tests use it; a tiny product falls back to fractions, a huge or non-finite one to a b + c."""
    a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        out = th + _round_to_odd_sum(np.ascontiguousarray(tl), np.ascontiguousarray(ul))
        mag = np.maximum(np.abs(uh), np.abs(c))
        plain = a * b + c
        wild = ~np.isfinite(plain) | (mag > 1e290) | (np.abs(a) > 1e150) | (np.abs(b) > 1e150)     # (overflow: where it matters to nobody)
        unsafe = ~wild & (np.abs(uh) < 1e-270) & (uh != 0.0)
    out = np.where(wild, plain, out)
    if np.any(unsafe):
        out[unsafe] = fma_exact(a[unsafe], b[unsafe], c[unsafe])
    return out


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    return fma_exact(a, b, c) if a.size <= FMA_EXACT_MAX else fma_fast(a, b, c)


def fma_plain(a, b, c):
    """a b + c with two roundings: for the statistical guards, where the last bit does not matter."""
    return a * b + c


# ---- the proposal g = N(m, L L^T) ------------------------------------------------------------------------------------------------------
def cholesky(V):
    """The lower factor of V in plain double, row by row, each inner product in index order, no fma; raises ValueError naming the
    parameter whose pivot is not positive and finite."""
    V = np.asarray(V, dtype=np.float64)
    d = V.shape[0]
    L = np.zeros((d, d))
    for p in range(d):
        for q in range(p):
            acc = float(V[p, q])
            for k in range(q):
                acc = acc - float(L[p, k]) * float(L[q, k])
            L[p, q] = acc / float(L[q, q])
        acc = float(V[p, p])
        for k in range(p):
            acc = acc - float(L[p, k]) * float(L[p, k])
        if not (acc > 0.0) or not (acc < math.inf):
            raise ValueError(f"pivot of parameter {p} is {acc}")
        L[p, p] = math.sqrt(acc)
    return L


def c_g(L):
    """sum dm_log(L_pp) + (d / 2) log 2 pi, added in index order."""
    d = L.shape[0]
    cg = 0.0
    for p in range(d):
        cg = cg + float(O.dm_log(np.array([L[p, p]]))[0])
    return cg + (0.5 * d) * LOG_2PI


def logg_of_z(z, cg, fma=fma):
    """z: (n, d) -> log g: s = sum z_p^2 by fma from 0 in index order, -0.5 s - c_g."""
    s = np.zeros(z.shape[0])
    for p in range(z.shape[1]):
        s = fma(z[:, p], z[:, p], s)
    return -0.5 * s - cg


def solve_z(x, m, L, fma=fma):
    """x: (n, d) -> z with L z = x - m: acc = x_p - m_p; acc = fma(-L_pq, z_q, acc) for q < p; z_p = acc / L_pp."""
    n, d = x.shape
    z = np.empty((n, d))
    for p in range(d):
        acc = x[:, p] - m[p]
        for q in range(p):
            acc = fma(-L[p, q], z[:, q], acc)
        z[:, p] = acc / L[p, p]
    return z


def posterior_a1(chain, log_obj, m, L, fma=fma):
    """chain: N x d x w, log_obj: N x w -> a1 = log_obj - log g(x), N x w."""
    N, d, w = chain.shape
    x = np.ascontiguousarray(np.transpose(chain, (0, 2, 1)).reshape(N * w, d))
    with np.errstate(all="ignore"):
        return log_obj - logg_of_z(solve_z(x, m, L, fma), c_g(L), fma).reshape(N, w)


def proposal_z(seed, Np, wp, d):
    """The normals of draw (c, t): the Box-Muller pairs of Philox blocks t B .. t B + B - 1 of stream (seed, c), B = ceil(d / 2);
    for odd d the last value is unused.  Np x d x wp."""
    B = (d + 1) // 2
    z = np.empty((Np, 2 * B, wp))
    for c in range(Np):
        for t in range(wp):
            for k in range(B):
                r1, r2 = O.draw_block(seed, c, t * B + k)
                z[c, 2 * k, t], z[c, 2 * k + 1, t] = O.normal_pair(r1, r2)
    return z[:, :d, :]


def proposal_x(z, m, L, fma=fma):
    """z: Np x d x wp -> x_p = m_p + sum_{q <= p} L_pq z_q by fma in index order; Np x d x wp."""
    Np, d, wp = z.shape
    zz = np.ascontiguousarray(np.transpose(z, (0, 2, 1)).reshape(Np * wp, d))
    x = np.empty((Np * wp, d))
    for p in range(d):
        acc = np.full(Np * wp, float(m[p]))
        for q in range(p + 1):
            acc = fma(L[p, q], zz[:, q], acc)
        x[:, p] = acc
    return np.asfortranarray(np.transpose(x.reshape(Np, wp, d), (0, 2, 1)))


def proposal(seed, Np, wp, m, L, fma=fma, z=None):
    """(x: Np x d x wp, logg: Np x wp) of the proposal's draws, from the normals drawn (no solve)."""
    d = len(m)
    z = proposal_z(seed, Np, wp, d) if z is None else z
    x = proposal_x(z, m, L, fma)
    zz = np.ascontiguousarray(np.transpose(z, (0, 2, 1)).reshape(Np * wp, d))
    return x, logg_of_z(zz, c_g(L), fma).reshape(Np, wp)


def rows_of(x):
    """Np x d x wp -> (Np wp) x d, draw j = c + Np t at row c wp + t (the order posterior_a1 and proposal use before reshaping)."""
    Np, d, wp = x.shape
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)).reshape(Np * wp, d))


# ---- the iteration -------------------------------------------------------------------------------------------------------------------
def _flat(a):
    """An N x w (or flat) array in the device's order: draw i = c + N t."""
    return np.ravel(np.asarray(a, dtype=np.float64), order="F")


def _weights(neff, n1, n2):
    ne = float(neff) if neff is not None and neff > 0 else float(n1)
    s1 = ne / (ne + float(n2))
    return s1, 1.0 - s1


_NAN_RESULT = dict(logml=float("nan"), converged=False, moments=np.full(4, np.nan), f2=None)


def _refused(a1, a2):
    return bool(not np.all(np.isfinite(a1)) or np.any(a2 == np.inf))


def iterate_ext(a1, a2, neff=None, tol=1e-10, max_iter=1000, use=None):
    """The iteration in the wide number system: dict(logml, iterations, converged, moments, n_nan, f2, deltas).  deltas: every
    |rho' - rho| as a float, for the worlds' conditions."""
    W = lr._Wide(use)
    a1, a2 = _flat(a1), _flat(a2)
    n1, n2 = a1.size, a2.size
    n_nan = int(np.isnan(a2).sum())
    if _refused(a1, a2):
        return dict(_NAN_RESULT, iterations=0, n_nan=n_nan, deltas=[])
    s1, s2 = (W.scalar(v) for v in _weights(neff, n1, n2))
    live = np.isfinite(a2)                               # (-inf and NaN entries: f1 = 0)
    a2w, a1w = W.lift(a2[live]), W.lift(a1)
    one = W.scalar(1.0)

    def f_of(rho):
        return one / (s1 + s2 * W.exp(rho - a2w)), one / (s1 * W.exp(a1w - rho) + s2)

    rho = W.scalar(float(a1.max()))
    it, converged, deltas, nan = 0, False, [], False
    while True:
        f1, f2 = f_of(rho)
        m1, m2 = f1.sum() / n2, f2.sum() / n1
        if not (m1 > 0) or not (m2 > 0):
            nan = True
            break
        new = rho + W.log(np.array([m1]))[0] - W.log(np.array([m2]))[0]
        delta = float(abs(new - rho))
        deltas.append(delta)
        rho, it = new, it + 1
        if delta <= tol:
            converged = True
            break
        if it >= max_iter:
            break
    if nan:
        return dict(_NAN_RESULT, iterations=it, n_nan=n_nan, deltas=deltas)
    f1, f2 = f_of(rho)
    m1, m2 = f1.sum() / n2, f2.sum() / n1
    # (the n2 - live.sum() zeros of f1 enter the two-pass variance with deviation -m1)
    v1 = (((f1 - m1) * (f1 - m1)).sum() + (n2 - int(live.sum())) * (m1 * m1)) / n2
    v2 = ((f2 - m2) * (f2 - m2)).sum() / n1
    return dict(logml=float(rho), iterations=it, converged=converged, moments=np.array([float(m1), float(v1), float(m2), float(v2)]),
                n_nan=n_nan, f2=np.array([float(v) for v in f2]), deltas=deltas)


def iterate_f64(a1, a2, neff=None, tol=1e-10, max_iter=1000):
    """The iteration in float64 in the device's order (bridge_sum_kernel, bridge_finish_kernel): the same dict without deltas."""
    a1, a2 = _flat(a1), _flat(a2)
    n1, n2 = a1.size, a2.size
    n_nan = int(np.isnan(a2).sum())
    s1, s2 = _weights(neff, n1, n2)
    nan2 = np.isnan(a2)

    def f_of(rho):
        with np.errstate(all="ignore"):
            f1 = np.where(nan2, 0.0, 1.0 / (s1 + s2 * np.exp(rho - a2)))
            f2 = 1.0 / (s1 * np.exp(a1 - rho) + s2)
        return f1, f2

    rho = float(np.fmax.reduce(a1)) if n1 else float("nan")
    if _refused(a1, a2):
        return dict(_NAN_RESULT, iterations=0, n_nan=n_nan)
    it, converged = 0, False
    mean = [0.0, 0.0]
    while True:
        f1, f2 = f_of(rho)
        mean = [lr._tile_sum(f1) / float(n2), lr._tile_sum(f2) / float(n1)]
        if not (mean[0] > 0.0) or not (mean[1] > 0.0):
            return dict(_NAN_RESULT, iterations=it, n_nan=n_nan)
        new = (rho + math.log(mean[0])) - math.log(mean[1])
        it += 1
        delta, rho = abs(new - rho), new
        if delta <= tol:
            converged = True
            break
        if it >= max_iter:
            break
    f1, f2 = f_of(rho)
    mom = []
    for f, n, shift in ((f1, n2, mean[0]), (f2, n1, mean[1])):
        dv = f - shift
        ms = lr._tile_sum(dv) / float(n)
        var = lr._tile_sum(dv * dv) / float(n) - ms * ms
        mom += [shift + ms, var if var > 0.0 else 0.0]
    return dict(logml=rho, iterations=it, converged=converged, moments=np.array(mom), n_nan=n_nan, f2=f2)


def se_of(moments, n2, ess_f2):
    """sqrt(var f1 / (N2 mean f1^2) + var f2 / (ESS(f2) mean f2^2)) in float64, the operations of demcz_bridge."""
    m1, v1, m2, v2 = (float(v) for v in moments)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v1) / (np.float64(n2) * (np.float64(m1) * m1)) + np.float64(v2) / (np.float64(ess_f2) * (np.float64(m2) * m2))))


def se_ext(moments, n2, ess_f2, use=None):
    W = lr._Wide(use)
    m1, v1, m2, v2 = (W.scalar(v) for v in moments)
    return float(W.sqrt(np.array([v1 / (n2 * (m1 * m1)) + v2 / (W.scalar(ess_f2) * (m2 * m2))]))[0])


def ess_of_f2(f2, N):
    """(ESS, margin) of f2 as a one-column history of N chains (ess_reference, the wide number system)."""
    f2 = np.asarray(f2, dtype=np.float64)
    e = er.ess(np.asfortranarray(f2.reshape(N, 1, -1, order="F")))
    return float(e.ess[0]), float(e.margin[0]), e


def errors(got, ref):
    """dict(logml, moments) of a result `got` (logml, moments) against a reference dict, in the tolerances' units."""
    gl, rl = float(got["logml"]), float(ref["logml"])
    out = dict(logml=abs(gl - rl) / max(1.0, abs(rl)))
    rm = np.asarray(ref["moments"], dtype=np.float64)
    out["moments"] = float(np.max(np.abs(np.asarray(got["moments"], dtype=np.float64) - rm) / np.maximum(np.abs(rm), 1e-300)))
    return out


def cholesky_error(L, V):
    V = np.asarray(V, dtype=np.float64)
    sd = np.sqrt(np.diag(V))
    return float(np.max(np.abs(L @ L.T - V) / np.outer(sd, sd)))


# ---- the whole pipeline in float64, for the statistical guards ------------------------------------------------------------------------
def bridge_f64(chain, log_obj, logobj, rng=None, seed=None, neff=None, tol=1e-10, max_iter=1000, m=None, L=None, fma=fma_plain):
    """demcz_bridge restated: the window is the whole history; its first half fits (m, V) unless m and L are given.  The proposal's
    normals come from `rng` (a NumPy generator: the guards) or from Philox stream `seed` (the bit-exact twin of the device's draws,
    with fma=fma).  logobj: (n, d) rows -> log-densities.  Returns the Bridge fields as a dict, plus a1, a2 and the iteration."""
    N, d, w = chain.shape
    h = w // 2
    if m is None:
        fit = rows_of(chain[:, :, :h])
        m = fit.mean(axis=0)
        L = cholesky(np.atleast_2d(np.cov(fit, rowvar=False)))
    a1 = posterior_a1(chain[:, :, h:], log_obj[:, h:], m, L, fma)
    z = np.asfortranarray(rng.standard_normal((N, d, w - h))) if rng is not None else None
    x, logg = proposal(seed, N, w - h, m, L, fma, z)
    with np.errstate(all="ignore"):
        a2 = np.asarray(logobj(rows_of(x)), dtype=np.float64).reshape(N, w - h) - logg
    it = iterate_f64(a1, a2, neff, tol, max_iter)
    out = dict(it, a1=a1, a2=a2, mean=m, L=L, n_post=a1.size, n_prop=a2.size, ess_f2=float("nan"), se_logml=float("nan"))
    if it["f2"] is not None and w - h >= 4:
        out["ess_f2"] = ess_of_f2(it["f2"], N)[0]
        out["se_logml"] = se_of(it["moments"], a2.size, out["ess_f2"])
    return out
