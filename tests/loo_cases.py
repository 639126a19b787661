"""The worlds of the PSIS-LOO / WAIC tests: arrays of pointwise log-likelihoods (N x nobs x G, column-major) built so that every path
of demcz_kernels_loo.h is taken -- and the pointwise programs with their NumPy twins.  tests/test_loo_cases.py holds every world
to its condition with the reference alone (tests/loo_reference.py); tests/test_gpu_loo.py runs the device over them.

A world is dict(name, loglik, r_eff (None or nobs values), window (None, or (g_from, g_to) inside the history), expect), where
expect maps a column to what the reference must say of it: n_tail=..., no_fit=True, m_min=..., n_below_M=True, khat_above=...,
khat_below=..., constant=value, bad=True, floor=True (the cutoff is log DBL_MIN).
"""
import functools
import math

import numpy as np

import loo_reference as lr


def _normal_loglik(rng, N, nobs, G, scale=1.0, offset=0.0):
    """Gaussian log-likelihoods of nobs observations at N x G independent posterior draws of a mean."""
    y = rng.normal(0.3, 1.0, nobs)
    theta = rng.normal(y.mean(), scale / math.sqrt(nobs), (N, 1, G))
    a = -0.5 * (y[None, :, None] - theta) ** 2 - 0.9189385332046727 + offset
    return np.asfortranarray(a)


def _column_with_tail(rng, N, G, n):
    """A column of S = N G values whose sorted front is n distinct values below a run of ties that covers index M: tail length n."""
    S = N * G
    M = lr.tail_cap(S)
    assert n <= M
    run = M - n + 7                                               # the ties stand at sorted positions n .. n + run - 1, around M
    front = -3.0 - np.sort(rng.exponential(1.0, n))[::-1]         # n distinct values below -3
    rest = -3.0 + rng.exponential(0.7, S - n - run) + 1e-3
    col = np.concatenate([front, np.full(run, -3.0), rest])
    assert np.unique(front).size == n and col.size == S
    return rng.permutation(col)


def _as_world_column(col, N, G):
    return np.asfortranarray(col.reshape(G, N).T.reshape(N, 1, G))


def _low_accept(rng, N, G, p_accept):
    """Chains that move with probability p_accept a generation: runs of repeated draws, as rejected proposals leave them."""
    theta = np.empty((N, G))
    cur = rng.normal(0.0, 1.0, N)
    for g in range(G):
        move = rng.random(N) < p_accept
        cur = np.where(move, rng.normal(0.0, 1.0, N), cur)
        theta[:, g] = cur
    return np.asfortranarray((-0.5 * (1.7 - theta) ** 2 - 0.9189385332046727).reshape(N, 1, G))


@functools.lru_cache(maxsize=None)
def worlds():
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, loglik, expect, r_eff=None, window=None):
        out.append(dict(name=name, loglik=np.asfortranarray(loglik, dtype=np.float64), r_eff=r_eff, window=window, expect=expect))

    # tail lengths 4 (no fit) and 5 (the smallest fit): S = 400, M = 60
    for n in (4, 5):
        add(f"tail{n}", _as_world_column(_column_with_tail(rng, 16, 25, n), 16, 25), {0: dict(n_tail=n, no_fit=(n == 4))})
    # around one workgroup of lanes: S = 8000, M = 269
    assert lr.tail_cap(64 * 125) == 269
    for n in (255, 256, 257):
        add(f"tail{n}", _as_world_column(_column_with_tail(rng, 64, 125, n), 64, 125), {0: dict(n_tail=n)})
    # m >= 65 candidates: S = 168000, M = 1230, every value distinct
    assert lr.tail_cap(420 * 400) == 1230 and lr.candidates(1230) == 65 and lr.candidates(1224) == 64
    add("many_candidates", _normal_loglik(rng, 420, 1, 400), {0: dict(n_tail=1230, m_min=65)})
    # a chain that rarely moves: the cutoff falls inside a run of ties
    add("low_accept", _low_accept(rng, 32, 200, 0.08), {0: dict(n_below_M=True)})
    # constant, poisoned and clean columns side by side
    base = _normal_loglik(rng, 16, 7, 30)
    base[:, 1, :] = -1.25
    base[3, 2, 11] = np.nan
    base[0, 4, 0] = -np.inf
    base[15, 5, 29] = np.inf
    add("poisoned", base, {1: dict(constant=-1.25), 2: dict(bad=True), 4: dict(bad=True), 5: dict(bad=True)})
    clean = base.copy()
    clean[:, 2, :] = clean[:, 0, :]
    clean[:, 4, :] = clean[:, 3, :]
    clean[:, 5, :] = clean[:, 6, :]
    add("poisoned_clean_twin", clean, {1: dict(constant=-1.25)})
    # a heavy and a light column: ratios exp(-a) with a Pareto tail of shape 1.2, and bounded ratios (k = -1/2)
    N, G = 32, 100
    heavy = -1.2 * rng.exponential(1.0, (N, 1, G))
    light = -np.log(0.5 + 0.5 * rng.beta(1.0, 2.0, (N, 1, G)))
    add("heavy_light", np.concatenate([heavy, light], axis=1), {0: dict(khat_above=0.7), 1: dict(khat_below=0.0)})
    # log-likelihoods far from zero: exp(a) underflows, and the mean is 1e6 standard deviations from zero
    add("far_from_zero", np.concatenate([_normal_loglik(rng, 16, 2, 30, offset=-800.0),
                                         1e6 + 1e-3 * rng.normal(0.0, 1.0, (16, 1, 30))], axis=1), {})
    # a column wider than exp can span: lw_M is below log DBL_MIN, so the cutoff is the floor and the tail the 20 values within it
    # (first column, fitted), or only 3 of them (second column, no fit)
    wide = rng.normal(-1000.0, 50.0, (16, 2, 30))
    wide[:, 0, 0] = -5000.0 + 25.0 * np.arange(16)
    wide[:4, 0, 1] = -4990.0 + 30.0 * np.arange(4)
    wide[:3, 1, 0] = [-5000.0, -4700.0, -4400.0]
    add("floor_cut", wide, {0: dict(n_tail=20, floor=True), 1: dict(n_tail=3, no_fit=True, floor=True)})
    # per-observation r_eff
    add("r_eff", _normal_loglik(rng, 24, 3, 50), {}, r_eff=np.array([0.3, 1.7, 0.9]))
    # column counts around the chunk boundary
    for nobs in (1, 32, 33, 70):
        add(f"columns{nobs}", _normal_loglik(rng, 16, nobs, 30), {})
    # a window that starts inside the history and has odd length
    add("window", _normal_loglik(rng, 24, 5, 60), {}, window=(7, 51))
    return out


def window_of(world):
    """The N x nobs x w array the statistics are about."""
    a = world["loglik"]
    if world["window"] is None:
        return a
    g_from, g_to = world["window"]
    return a[:, :, g_from - 1:g_to]


@functools.lru_cache(maxsize=None)
def reference(i):
    """loo_reference.columns (the wide reference) of world i, computed once."""
    w = worlds()[i]
    return lr.columns(window_of(w), w["r_eff"])


@functools.lru_cache(maxsize=None)
def restatement(i, naive=False):
    w = worlds()[i]
    return lr.columns(window_of(w), w["r_eff"], how=lr.column_naive if naive else lr.column_f64)


# ---- pointwise programs and their twins (only +, -, * and written fma: the same doubles on the device and in NumPy) ---------------
def gaussian_program(demc, d, nobs, seed=0):
    """(PointwiseProgram, twin): observation i has a design row z_i of d entries and a response y_i in data; with the known
    precision tau the log-likelihood is c - 0.5 tau r^2, r = y_i - sum_p z_ip x_p summed in index order, the last step an fma."""
    rng = np.random.default_rng(1000 + 31 * d + nobs + seed)
    Z = np.round(rng.normal(0.0, 1.0, (nobs, d)), 3)
    y = np.round(rng.normal(0.0, 2.0, nobs), 3)
    data = np.concatenate([Z.ravel(), y])
    src = f"""
#define NOBS {nobs}
__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)
{{
    const double* z = data + i * DEMCZ_D;
    double mu = 0.0;
#pragma unroll
    for (int p = 0; p < DEMCZ_D; ++p) mu = mu + z[p] * x[p];
    const double r = data[(int64_t)NOBS * DEMCZ_D + i] - mu;
    return fma(-0.125 * r, r, -1.612085713764618);
}}
"""
    prog = demc.PointwiseProgram(src, d, nobs, data=data, names=[f"y{i}" for i in range(nobs)])

    def twin(chain, obs_from=0, obs_to=None):
        obs_to = nobs if obs_to is None else obs_to
        N, _, G = chain.shape
        out = np.empty((N, obs_to - obs_from, G), order="F")
        for k, i in enumerate(range(obs_from, obs_to)):
            mu = np.zeros((N, G))
            for p in range(d):
                mu = mu + Z[i, p] * chain[:, p, :]
            r = y[i] - mu
            out[:, k, :] = fma_exact(-0.125 * r, r, -1.612085713764618)
        return out

    return prog, twin


def fma_exact(a, b, c):
    """fma(a, b, c) elementwise, correctly rounded: a b + c in exact fractions, rounded once."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    from fractions import Fraction
    out = np.empty(a.shape)
    flat_a, flat_b, flat_o = a.ravel(), b.ravel(), out.ravel()
    for i in range(flat_a.size):
        flat_o[i] = float(Fraction(float(flat_a[i])) * Fraction(float(flat_b[i])) + Fraction(float(c)))
    return out


def chain_history(N, d, G, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.normal(0.0, 1.0, (N, d, G)))
