"""Extended-precision reference of the effective sample size (BDA3 section 11.5 / the Stan reference manual
on the split chains of Rhat_gelman, without rank normalisation), for test_ess_reference.py (which proves it against exact rational
arithmetic) and test_gpu_ess.py (which holds the device to it).

Everything is evaluated in stats_reference.backend()'s numbers (long double, or mpmath where long double is no wider than a
double), two-pass (split-chain means first, then the lagged products of the deviations), on data centred on chain 0's first
sample like stats_reference._centred: the autocovariance does not depend on a common shift, and the deviations from a split
chain's mean are then differences of numbers a few standard deviations in size, never of the offset.

The statistic, per parameter, with n = G // 2 samples per split chain and m = 2 N split chains (an odd window never reads its
last generation):

    c_j(t) = 1/n sum_{i=0}^{n-t-1} (x_ji - mean_j)(x_j,i+t - mean_j),  t = 0..L;  L = n - 1, or min(n - 1, max_lag) if max_lag > 0
    A(t) = 1/m sum_j c_j(t);  W = A(0) n/(n-1);  B/n = sum_j (mean_j - grand)^2 / (m-1);  var+ = A(0) + B/n
    rho_0 = 1, rho_t = 1 - (W - A(t))/var+;  P_k = rho_2k + rho_2k+1 while 2k+1 <= L
    the first k with !(P_k > 0) ends the sequence (not summed, converged = 1; a NaN pair makes tau NaN); otherwise
    P_k <- min(P_k, P_k-1) is added; lags run out: converged = 0
    tau = -1 + 2 sum P_k;  S = m n;  ESS = S/tau, and S log10(S) where tau < 1/log10(S)

`margin` is how far the stopping decisions are from flipping: the smallest pair that was summed and minus the stopping pair,
whichever is smaller (+inf where neither exists).
"""
import math
from collections import namedtuple

import numpy as np

import stats_reference as R

Ess = namedtuple("Ess", "A rho tau pairs converged ess varplus margin sums between n m L")


def lags(G, max_lag=0):
    n = G // 2
    return n - 1 if max_lag <= 0 else min(n - 1, int(max_lag))


def split_deviations(chain, use=None):
    """(dev, means, n, m): the 2N split chains' deviations from their own means, 2N x d x n, and those means (centred on the
    pivot), 2N x d x 1, in the backend's numbers."""
    Bk = R.backend(use)
    chain = np.asarray(chain, dtype=np.float64)
    N, d, G = chain.shape
    n = G // 2
    if n < 2:
        raise ValueError("the split chains need at least 4 generations")
    c, _ = R._centred(Bk, chain[:, :, :2 * n])
    cs = np.concatenate([c[:, :, :n], c[:, :, n:2 * n]], axis=0)
    means = R._mean(cs, (2,))
    return cs - means, means, n, 2 * N


def autocov_sums(chain, max_lag=0, use=None):
    """(sums, between): sums[p, t] = sum_j n c_j(t), d x (L + 1), and between[p] = sum_j (mean_j - grand)^2, extended."""
    dev, means, n, m = split_deviations(chain, use)
    L = lags(np.shape(chain)[2], max_lag)
    sums = np.stack([(dev[:, :, :n - t] * dev[:, :, t:]).sum(axis=(0, 2)) for t in range(L + 1)], axis=1)
    grand = R._mean(means, (0,))
    between = ((means - grand) ** 2).sum(axis=0).ravel()
    return sums, between


def finish(sums, between, n, m):
    """The finisher in the number system `sums` comes in (extended arrays, or float64 for the NumPy restatement of the device)."""
    sums, between = np.asarray(sums), np.asarray(between)
    d, nl = sums.shape
    L = nl - 1
    S = m * n
    A = sums / S
    W = A[:, 0] * n / (n - 1)
    vp = A[:, 0] + between / (m - 1)
    with np.errstate(all="ignore"):
        rho = np.stack([_div(W[p] - A[p], vp[p]) for p in range(d)])
    rho = 1 - rho
    rho[:, 0] = 1
    tau, ess = np.empty(d), np.empty(d)
    pairs, conv = np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int32)
    margin = np.full(d, np.inf)
    cap, floor_tau = S * math.log10(S), 1.0 / math.log10(S)
    for p in range(d):
        total, prev, k = 0, None, 0
        while 2 * k + 1 <= L:
            P = rho[p, 2 * k] + rho[p, 2 * k + 1]
            if not P > 0:
                conv[p] = 1
                if P != P:
                    total = P
                else:
                    margin[p] = min(margin[p], float(-P))
                break
            margin[p] = min(margin[p], float(P))
            if prev is not None and prev < P:
                P = prev
            total, prev, k = total + P, P, k + 1
        t = -1 + 2 * total
        pairs[p], tau[p] = k, float(t)
        with np.errstate(all="ignore"):
            ess[p] = cap if t < floor_tau else float(S / t)
    return A, rho, tau, pairs, conv, ess, vp, margin


def _div(a, b):
    """a / b elementwise with IEEE results for b = 0, in either number system."""
    a = np.asarray(a)
    if a.dtype != object:
        return a / b
    return R._MP.div(a, np.broadcast_to(np.asarray(b, dtype=object), a.shape))


def ess(chain, max_lag=0, use=None):
    """The whole statistic: an Ess tuple; A, rho, sums, between and varplus stay extended, the rest is rounded to float64."""
    chain = np.asarray(chain, dtype=np.float64)
    N, d, G = chain.shape
    n, m = G // 2, 2 * N
    sums, between = autocov_sums(chain, max_lag, use)
    A, rho, tau, pairs, conv, e, vp, margin = finish(sums, between, n, m)
    return Ess(A, rho, tau, pairs, conv, e, vp, margin, sums, between, n, m, sums.shape[1] - 1)


def ess_of_tau(tau, S):
    """What the library must return for a tau it returns: S / tau, or the cap -- in float64, an identity."""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(tau < 1.0 / math.log10(S), S * math.log10(S), S / tau)


# ---- tolerances: they follow from COV_RTOL, the project's bound for second moments -------------------------
ACOV_RTOL = R.COV_RTOL               # |dA_p(t)| <= 1e-9 A_p(0) for every lag, hence |d rho_t| <= 4e-9
TAU_ATOL_PER_LAG = 1e-8              # |d tau| <= 1e-8 (2 pairs + 1)
VARPLUS_RTOL = 1e-9
MARGIN = 1e-4                        # precondition of equal pairs / converged: a hundred times the rho bound


def acov_error(got_A, ref):
    """max over (p, t) of |got - A_p(t)| / A_p(0)."""
    A = R.to_float(ref.A)
    return float(np.max(np.abs(np.asarray(got_A) - A) / A[:, :1]))


def tau_error(got_tau, ref):
    """max over p of |got - tau_p| / (2 pairs_p + 1): the tolerance is TAU_ATOL_PER_LAG."""
    return float(np.max(np.abs(np.asarray(got_tau) - ref.tau) / (2 * ref.pairs + 1)))


def varplus_error(got, ref):
    vp = R.to_float(ref.varplus)
    return float(np.max(np.abs(np.asarray(got) - vp) / vp))
