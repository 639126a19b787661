"""The NumPy reference of the rank-normalised diagnostics, shared by test_rank_reference.py (no GPU) and
test_gpu_rank.py: average ranks with ties, a restatement of the device's logarithm (dm_log, fdlibm) with the integer work on uint64
views, a restatement of Wichura's AS 241 PPND16 with one rounded operation per line, and rank -> z as the library forms it.
NumPy float64 arithmetic rounds every elementwise operation once and fuses nothing, so the restatement can be held to the
library bit for bit."""
import numpy as np

# ---- average ranks -------------------------------------------------------------------------------------------------------------------
def values_ranked(x, center=None):
    """v = x, or fabs(x - center); then v + 0.0 (so that -0.0 ranks as +0.0)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v = x if center is None else np.abs(x - np.float64(center))
        return v + 0.0


def average_ranks(x, center=None):
    """1-based average ranks of the entries of a 1-d array among themselves: less + (equal + 1) / 2, ties by ==.  No NaN."""
    v = values_ranked(x, center)
    assert v.ndim == 1 and not np.isnan(v).any()
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    less = np.cumsum(cnt) - cnt
    return less[inv].astype(np.float64) + 0.5 * (cnt[inv] + 1).astype(np.float64)


# ---- dm_log --------------------------------------------------------------------------------------------------------------------------
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
      1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)


def dm_log(x):
    """Natural logarithm of positive normal doubles, the device's operation sequence."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    hx = b >> np.uint64(32)
    lx = b & np.uint64(0xFFFFFFFF)
    hx = (hx + np.uint64(0x3FF00000 - 0x3FE6A09E)) & np.uint64(0xFFFFFFFF)
    k = (hx >> np.uint64(20)).astype(np.int64) - 0x3FF
    hx = (hx & np.uint64(0x000FFFFF)) + np.uint64(0x3FE6A09E)
    xr = ((hx << np.uint64(32)) | lx).view(np.float64)
    f = xr - 1.0
    hfsq = 0.5 * f
    hfsq = hfsq * f
    s = 2.0 + f
    s = f / s
    z = s * s
    w = z * z
    t1 = w * LG[5]
    t1 = LG[3] + t1
    t1 = w * t1
    t1 = LG[1] + t1
    t1 = w * t1
    t2 = w * LG[6]
    t2 = LG[4] + t2
    t2 = w * t2
    t2 = LG[2] + t2
    t2 = w * t2
    t2 = LG[0] + t2
    t2 = z * t2
    R = t2 + t1
    dk = k.astype(np.float64)
    out = hfsq + R
    out = s * out
    lo = dk * LN2_LO
    out = out + lo
    out = out - hfsq
    out = out + f
    hi = dk * LN2_HI
    return out + hi


# ---- AS 241, PPND16 --------------------------------------------------------------------------------------------------------------------
A = (3.387132872796366608, 133.14166789178437745, 1971.5909503065514427, 13731.693765509461125, 45921.953931549871457,
     67265.770927008700853, 33430.575583588128105, 2509.0809287301226727)
B = (1.0, 42.313330701600911252, 687.1870074920579083, 5394.1960214247511077, 21213.794301586595867, 39307.89580009271061,
     28729.085735721942674, 5226.495278852854561)
C = (1.42343711074968357734, 4.6303378461565452959, 5.7694972214606914055, 3.64784832476320460504, 1.27045825245236838258,
     0.24178072517745061177, 0.0227238449892691845833, 7.7454501427834140764e-4)
D = (1.0, 2.05319162663775882187, 1.6763848301838038494, 0.68976733498510000455, 0.14810397642748007459,
     0.0151986665636164571966, 5.475938084995344946e-4, 1.05075007164441684324e-9)
E = (6.6579046435011037772, 5.4637849111641143699, 1.7848265399172913358, 0.29656057182850489123, 0.026532189526576123093,
     0.0012426609473880784386, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
F = (1.0, 0.59983220655588793769, 0.13692988092273580531, 0.0148753612908506148525, 7.868691311456132591e-4,
     1.8463183175100546818e-5, 1.4215117583164458887e-7, 2.04426310338993978564e-15)


def horner(coef, r):
    """coef[7] r^7 + ... + coef[0], from the top, a multiplication and an addition at a time."""
    acc = np.full(r.shape, coef[7])
    for c in coef[6::-1]:
        acc = acc * r
        acc = acc + c
    return acc


def ppnd16_lower(u):
    """The normal quantile of 0 < u <= 0.5 (so <= 0) by AS 241's PPND16."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    q = u - 0.5
    out = np.empty(u.shape)
    central = q >= -0.425
    if central.any():
        qc = q[central]
        r = qc * qc
        r = 0.180625 - r
        num = qc * horner(A, r)
        out[central] = num / horner(B, r)
    tail = ~central
    if tail.any():
        lg = dm_log(u[tail])
        r = np.sqrt(-lg)
        mid = r <= 5.0
        val = np.empty(r.shape)
        rm = r[mid] - 1.6
        val[mid] = horner(C, rm) / horner(D, rm)
        rf = r[~mid] - 5.0
        val[~mid] = horner(E, rf) / horner(F, rf)
        out[tail] = -val
    return out


def blom_u(r, S):
    """(upper, u): whether the rank lies above its mirror image S + 1 - r, and u = (min(r, S + 1 - r) - 0.375) / (S + 0.25)."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    S = np.float64(S)
    mirror = (S + 1.0) - r
    upper = r > mirror
    rl = np.where(upper, mirror, r)
    u = rl - 0.375
    return upper, u / (S + 0.25)


def rank_to_z(r, S):
    """The normal scores of average ranks r among S draws."""
    upper, u = blom_u(r, S)
    z = ppnd16_lower(u)
    return np.where(upper, -z, z)


# ---- a whole history -----------------------------------------------------------------------------------------------------------------
def ranks_of_chain(chain, center=None):
    """N x d x G average ranks per parameter over all N G draws; a parameter whose values ranked hold a NaN is NaN throughout."""
    chain = np.asarray(chain, dtype=np.float64)
    N, d, G = chain.shape
    out = np.empty((N, d, G), order="F")
    for p in range(d):
        c = None if center is None else center[p]
        v = values_ranked(chain[:, p, :], c)
        if np.isnan(v).any():
            out[:, p, :] = np.nan
        else:
            out[:, p, :] = average_ranks(np.ascontiguousarray(chain[:, p, :]).ravel(), c).reshape(N, G)
    return out


def z_of_ranks(ranks):
    """rank_to_z over an N x d x G array of ranks (S = N G); NaN stays NaN."""
    N, d, G = ranks.shape
    out = np.full((N, d, G), np.nan, order="F")
    ok = ~np.isnan(ranks)
    out[ok] = rank_to_z(ranks[ok], N * G)
    return out


def indicator_le(chain, thr):
    """N x (d nthr) x G: column p + d u is (x[:, p, :] <= thr[p, u]) as 1.0 / 0.0, NaN where x is NaN."""
    chain = np.asarray(chain, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    thr = thr.reshape(chain.shape[1], -1, order="F")
    N, d, G = chain.shape
    out = np.empty((N, d * thr.shape[1], G), order="F")
    for u in range(thr.shape[1]):
        for p in range(d):
            x = chain[:, p, :]
            with np.errstate(invalid="ignore"):
                out[:, p + d * u, :] = np.where(np.isnan(x), np.nan, (x <= thr[p, u]).astype(np.float64))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the statistic, composed from the existing references ----------------------------------------------------------------------------
def diagnostics(chain):
    """(rhat_rank, ess_bulk, ess_tail, parts) of an N x d x G history, as demcz_rank_diagnostics composes them: the type-7
    quantiles of quantile_cases, the extended-precision split R-hat of stats_reference and ESS of ess_reference, fed the restated
    normal scores and the indicators."""
    import ess_reference as E
    import quantile_cases as Q
    import stats_reference as SR
    chain = np.asarray(chain, dtype=np.float64)
    d = chain.shape[1]
    q = Q.reference(chain, (0.05, 0.5, 0.95)).q
    zb = z_of_ranks(ranks_of_chain(chain))
    zf = z_of_ranks(ranks_of_chain(chain, center=q[:, 1]))
    with np.errstate(all="ignore"):
        rb, rf = SR.rhat_gelman(zb), SR.rhat_gelman(zf)
        rhat = np.where(np.isnan(rb) | np.isnan(rf), np.nan, np.maximum(rb, rf))
        bulk = E.ess(zb)
        tails = E.ess(indicator_le(chain, np.stack([q[:, 0], q[:, 2]], axis=1)))
        lo, hi = tails.ess[:d], tails.ess[d:]
        tail = np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.minimum(lo, hi))
    return rhat, bulk.ess, tail, dict(q=q, zb=zb, zf=zf, rhat_bulk=rb, rhat_folded=rf, bulk=bulk, tails=tails)
