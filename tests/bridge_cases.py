"""The worlds the bridge-sampling iteration is tested on (tests/test_bridge_cases.py without a GPU, tests/test_gpu_bridge.py on
the device): pairs (a1, a2) of log ratios, a few thousand draws at most, each with the arguments of the iteration.

A world is made from a d-dimensional normal posterior with an unnormalised log-density whose log Z is known, exact independent
draws of it as the N x w posterior side, and a normal proposal -- fitted, too narrow, too wide -- drawn by NumPy as the Np x wp
proposal side.  Nothing here is bit-exact: the worlds are data.  a1 is N x w, a2 is Np x wp, both in the device's order
(draw i = c + N t), so that f2 has chains for demcz_ess to split.

`converges` worlds satisfy the conditions test_bridge_cases.py holds the wide reference to -- the last change is <= tol / 4 and
the one before it >= 4 tol -- so that the number of updates is the same in any arithmetic that is good to a few ulp.  Where the
default tol = 1e-10 falls too close to one of the reference's changes, the world carries another tol."""
import functools

import numpy as np

import bridge_reference as br
from oracle_engine import OracleEngine

N_CH, W_IT = 16, 150          # 2400 posterior draws: two full tiles of 1024 and a part of a third


def _gauss_world(seed, d=3, scale=1.0, offset=0.0, Np=N_CH, wp=W_IT, lower=None):
    """(a1, a2): posterior N(0, I) with log_obj = offset - |x|^2 / 2 (log Z = offset + d/2 log 2 pi), or that density cut to
    x_0 >= lower (log Z then adds log P(x_0 >= lower)); the proposal is N(fitted mean, (scale * fitted sd)^2) per coordinate."""
    rng = np.random.default_rng(seed)
    n1, n2 = N_CH * W_IT, Np * wp
    xs = rng.standard_normal((2 * n1, d))
    if lower is not None:
        x0 = rng.standard_normal(8 * n1)
        xs[:, 0] = x0[x0 >= lower][:2 * n1]
    fit, post = xs[:n1], xs[n1:]
    m, sd = fit.mean(axis=0), fit.std(axis=0) * scale
    if lower is not None:
        m[0], sd[0] = lower, 1.0                          # the proposal straddles the boundary: half its draws fall outside

    def logobj(x):
        lp = offset - 0.5 * (x * x).sum(axis=1)
        return lp if lower is None else np.where(x[:, 0] >= lower, lp, -np.inf)

    def logg(x):
        z = (x - m) / sd
        return -0.5 * (z * z).sum(axis=1) - np.log(sd).sum() - 0.5 * d * br.LOG_2PI

    prop = m + sd * rng.standard_normal((n2, d))
    a1 = np.asfortranarray((logobj(post) - logg(post)).reshape(N_CH, W_IT, order="F"))
    a2 = np.asfortranarray((logobj(prop) - logg(prop)).reshape(Np, wp, order="F"))
    return a1, a2


@functools.lru_cache(maxsize=None)
def worlds():
    out = []

    def add(name, a1, a2, nan=False, converges=True, **args):
        args.setdefault("tol", 1e-10)
        args.setdefault("max_iter", 1000)
        args.setdefault("neff", None)
        out.append(dict(name=name, a1=a1, a2=a2, nan=nan, converges=converges and not nan, args=args))

    add("well_matched", *_gauss_world(1))
    add("narrow", *_gauss_world(2, scale=0.5))
    add("wide", *_gauss_world(3, scale=2.5))
    # bounded support: the posterior lives on x_0 >= 0, half the proposal's draws fall outside and have a2 = -inf
    a1, a2 = _gauss_world(4, lower=0.0)
    assert 0.3 < np.mean(np.isneginf(a2)) < 0.7
    add("half_outside", a1, a2, tol=1e-11)                           # (the reference's changes: ... 3.2e-10, 2.2e-13)
    add("offset_plus", *_gauss_world(5, offset=1e4), tol=2e-11)      # (... 3.5e-10, 2.0e-14; an ulp of rho is 1.8e-12)
    add("offset_minus", *_gauss_world(6, offset=-1e4))
    add("more_proposal", *_gauss_world(7, Np=23, wp=211))            # N2 = 4853 != N1 = 2400
    add("fewer_proposal", *_gauss_world(8, Np=9, wp=77))             # N2 = 693
    a1, a2 = _gauss_world(9)
    add("neff_seventh", a1, a2, neff=a1.size / 7.0, tol=2e-11)       # (... 2.2e-10, 9.9e-15)
    a1, a2 = _gauss_world(10)
    a2 = a2.copy(order="F")
    a2.T.reshape(-1)[[3, 1024, 2399]] = np.nan                       # counted in n_nan, taken as -inf
    add("nan_in_a2", a1, a2)
    a1, a2 = _gauss_world(11, scale=0.5)
    add("max_iter_3", a1, a2, converges=False, max_iter=3)
    # each of these gives NaN
    a1, a2 = _gauss_world(12)
    b = a2.copy(order="F"); b[5, 7] = np.inf
    add("inf_in_a2", a1, b, nan=True)
    b = a1.copy(order="F"); b[2, 140] = -np.inf
    add("neginf_in_a1", b, a2, nan=True)
    b = a1.copy(order="F"); b[15, 149] = np.nan
    add("nan_in_a1", b, a2, nan=True)
    add("all_outside", a1, np.full_like(a2, -np.inf), nan=True)
    return out


def names():
    return [w["name"] for w in worlds()]


@functools.lru_cache(maxsize=None)
def reference(i):
    """bridge_reference.iterate_ext (the wide reference) of world i, computed once."""
    w = worlds()[i]
    return br.iterate_ext(w["a1"], w["a2"], **w["args"])


@functools.lru_cache(maxsize=None)
def restatement(i):
    w = worlds()[i]
    return br.iterate_f64(w["a1"], w["a2"], **w["args"])


@functools.lru_cache(maxsize=None)
def reference_se(i):
    """(se_logml, ESS(f2), its margin) of world i in the wide number system; NaN worlds give NaN."""
    ref = reference(i)
    if ref["f2"] is None:
        return float("nan"), float("nan"), float("nan")
    ess, margin, _ = br.ess_of_f2(ref["f2"], worlds()[i]["a1"].shape[0])
    return br.se_ext(ref["moments"], worlds()[i]["a2"].size, ess), ess, margin


# ---- the end-to-end world: a history of the sampler itself ------------------------------------------------------------------------
E2E = dict(d=5, N=64, G=600, window=(201, 600), seed=2024)


@functools.lru_cache(maxsize=None)
def oracle_history():
    """chain, log_obj of the end-to-end world: the MvNormal workload at d = 5 with 64 chains for 600 generations on the CPU
    oracle, which the device reproduces bit for bit (tests/test_gpu_parity.py); and the oracle's problem, for its log-density."""
    import demc_jl_amd as demc
    w = demc.workloads.mvnormal_problem(E2E["d"], E2E["N"])
    M0 = w["Zinit"].shape[0]
    e = OracleEngine(N=E2E["N"], d=E2E["d"], K=w["K"], Mcap=M0 + E2E["N"] * (E2E["G"] // w["K"] + 1), Gcap=E2E["G"],
                     blockindex=[range(E2E["d"])], eps_scale=w["eps_scale"], seed=E2E["seed"], target=w["target"])
    e.set_state(w["Zinit"][-E2E["N"]:], None, w["Zinit"])
    e.run(1, E2E["G"], w["gamma"])
    chain, log_obj = e.get_history(1, E2E["G"])
    return w, e.prob, chain, log_obj
