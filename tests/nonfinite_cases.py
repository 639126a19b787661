"""Inputs shared by test_nonfinite_reference.py (which checks, on the oracle alone, that they are what the GPU tests assume) and
test_gpu_nonfinite.py (which runs them through every kernel layout): the rows of test_gpu_kernel_choice.py's table on a poisoned
starting population, and three worlds in which the log-density's arithmetic runs in the subnormal range."""
import numpy as np

import demc_jl_amd as demc
from helpers import oracle_sample, poisoned_population
from test_gpu_kernel_choice import CASES, _problem

BUILTIN_ROWS = [c for c, v in CASES.items() if v[0] != "prog"]
RUN_SEED = 11
POPULATION_SEED = 3
# rows whose oracle run misses a condition of test_nonfinite_reference.py at POPULATION_SEED get another seed here (never a weaker bound)
POPULATION_SEEDS = {}


def pieces(K):
    """observe_case's three calls: generations 1..4K, three more, then 2K tempered ones."""
    return [(1, 4 * K), (4 * K + 1, 4 * K + 3), (4 * K + 4, 6 * K + 3)]


def row_inputs(case):
    """A table row on poisoned_population, with a subnormal eps_scale[0].  T holds the temperatures of the third call only."""
    kind, d, N, K, lanes, blocks, nobs = CASES[case]
    w = _problem(kind, d, N, nobs)
    eps = np.array(w["eps_scale"], dtype=np.float64)
    eps[0] = 1e-320
    T = np.array([demc.tempbaseline(g, 2 * K, 3, 1e-3) for g in range(1, 2 * K + 1)])
    return dict(case=case, target=w["target"], gamma=w["gamma"], d=d, N=N, K=K, G=6 * K + 3, lanes=lanes,
                blocks=[list(b) for b in blocks] if blocks else None, eps=eps, T=T,
                Zinit=poisoned_population(d, N, POPULATION_SEEDS.get(case, POPULATION_SEED)), seed=RUN_SEED)


def full_temperatures(r):
    """One temperature per generation for a single oracle run: dividing by 1.0 is the identity on every double, so the plain calls
    are tempered at 1.0."""
    return np.concatenate([np.ones(r["G"] - len(r["T"])), r["T"]])


def reference(oracle, r):
    return oracle_sample(oracle, r["target"], r["Zinit"], r["N"], r["K"], r["G"], r["blocks"], r["eps"], r["gamma"], r["seed"],
                         temperature=r["temperature"] if "temperature" in r else full_temperatures(r))


# ---- subnormal worlds --------------------------------------------------------------------------------------------------------
ISO_SCALE = 2.0 ** -535          # residuals of 2^-535: their squares, and every log_obj, are subnormal
LR_SCALE = 2.0 ** -535           # the same through the regression's design
MVN_SCALE = 2.0 ** -1040         # states and increments are subnormal, q underflows to 0 and log_obj is the constant c0; every proposal
                                 # is accepted (log u < 0) while no log_obj changes.  (2^-1040 is the scale first tried: the oracle's
                                 # run is not degenerate there, every chain moves.)
WORLD_ROWS = {
    "iso": ["lane1_iso_d10", "ml8_iso_d10", "split_iso_d10", "wave_iso_d6"],
    "lr": ["lane1_lr_d10", "ml16_lr_d10", "split_lr_d10_lr8s", "ml16_lr_d7_coop"],
    "mvn": ["wave_mvn_d5", "wave_mvn_d20", "mlb16_mvn_d20_4x5", "split_mvn_d5"],
}
WORLD_CASES = [(world, case, tempered) for world, rows in WORLD_ROWS.items() for case in rows for tempered in (False, True)]


def world_inputs(world, case, tempered):
    kind, d, N, K, lanes, blocks, nobs = CASES[case]
    assert kind == world
    w = _problem(kind, d, N, nobs)
    Zinit, eps = np.array(w["Zinit"], order="F"), np.array(w["eps_scale"], dtype=np.float64)
    if world == "iso":
        target, Zinit, eps = demc.IsoQuadTarget(np.zeros(d)), Zinit * ISO_SCALE, 1e-3 * ISO_SCALE * np.ones(d)
    elif world == "lr":
        target = demc.LinRegSSETarget(w["design"] * LR_SCALE, np.zeros(nobs))
    else:
        target, Zinit, eps = demc.MvNormalTarget(np.zeros(d), w["Sigma"]), Zinit * MVN_SCALE, eps * MVN_SCALE
    G = 6 * K + 3
    T = np.array([demc.tempbaseline(g, G, 3, 1e-3) for g in range(1, G + 1)]) if tempered else None
    return dict(case=case, target=target, gamma=w["gamma"], d=d, N=N, K=K, G=G, lanes=lanes,
                blocks=[list(b) for b in blocks] if blocks else None, eps=eps, temperature=T, Zinit=Zinit, seed=RUN_SEED)


def subnormal_share(a):
    a = np.abs(np.asarray(a))
    return np.count_nonzero((a > 0) & (a < np.finfo(np.float64).tiny)) / a.size


def chains_that_move(ref, X0):
    """Chains whose state differs from the one before it at some generation (NaN coordinates compared as equal to themselves)."""
    hist = np.concatenate([np.asarray(X0)[:, :, None], ref["chain"]], axis=2)
    a, b = hist[:, :, 1:], hist[:, :, :-1]
    differs = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return differs.any(axis=(1, 2))


# ---- program targets -----------------------------------------------------------------------------------------------------------
PROGRAM_K, PROGRAM_G, PROGRAM_CALLS = 5, 45, [(1, 3), (4, 23), (24, 45)]
PROGRAM_GRID = [(name, d, N, tempered)
                for name in ("box", "box_poisoned", "sqrtdom", "pole", "trips")
                for d in (2, 5, 7, 20) for N in (64, 301) for tempered in (False, True)]
# the pole x[1] > t: a few chains of a standard normal population start in it or walk into it, and (it is absorbing, and the steps
# are longest at small d) more than half are still outside it after the 45 generations
POLE_T = {2: 2.8, 5: 2.3, 7: 2.0, 20: 2.0}


def program_inputs(name, d, N, tempered):
    """(program, its Python twin, Zinit, ...) of a case of PROGRAM_GRID.  The clean populations are standard normal; BOX's sides
    and SQRTDOM's edge are placed so that about a quarter of such a population lies outside the support."""
    from statistics import NormalDist
    import program_texts as P
    K, G = PROGRAM_K, PROGRAM_G
    Zinit = np.asfortranarray(np.random.default_rng(1000 * d + N).standard_normal((2 * N + 40, d)))
    eps, gamma = 1e-3 * np.ones(d), 1.0
    if name in ("box", "box_poisoned"):
        c, h = np.zeros(d), np.full(d, NormalDist().inv_cdf(0.5 + 0.5 * 0.75 ** (1.0 / d)))          # P(inside)^d = 3/4
        target, twin = P.box_program(c, h), P.box_closure(c, h)
        if name == "box_poisoned":
            Zinit = poisoned_population(d, N, POPULATION_SEED)
            eps[0] = 1e-320
    elif name == "sqrtdom":
        a, b = NormalDist().inv_cdf(0.25), 1.0
        target, twin = P.sqrtdom_program(d, a, b), P.sqrtdom_closure(d, a, b)
    elif name == "pole":
        target, twin = P.pole_program(d, POLE_T[d]), P.pole_closure(d, POLE_T[d])
    else:
        target, twin = P.trips_program(d), P.trips_closure(d)
    T = np.array([demc.tempbaseline(g, G, 3, 1e-3) for g in range(1, G + 1)]) if tempered else None
    return dict(name=name, target=target, twin=twin, d=d, N=N, K=K, G=G, Zinit=Zinit, eps=eps, gamma=gamma, temperature=T, seed=RUN_SEED)


def program_reference(oracle, r):
    from helpers import oracle_sample_logobj
    ref = oracle_sample_logobj(oracle, r["twin"], r["Zinit"], r["N"], r["K"], r["G"], None, r["eps"], r["gamma"], r["seed"],
                               temperature=r["temperature"])
    ref["logp0"] = np.array([r["twin"]([float(v) for v in x]) for x in r["Zinit"][-r["N"]:]])
    return ref


def program_reference_facts(r, ref):
    """What the reference run of a program case did, for the conditions the tests put on it."""
    N = r["N"]
    lp_hist = np.concatenate([ref["logp0"][:, None], ref["log_obj"]], axis=1)
    outside0 = ~np.isfinite(ref["logp0"])
    finite_before = np.isfinite(lp_hist[:, :-1])
    return dict(
        outside_at_start=int(outside0.sum()),
        entered=int((outside0 & np.isfinite(lp_hist[:, -1])).sum()),                    # started outside the support, ended inside
        finite_chain_rejected_outside=int((finite_before & ~np.isfinite(ref["proposed"][:, :, 0])).sum()),
        moved=int(np.count_nonzero(chains_that_move(ref, r["Zinit"][-N:]))),
        captured=int(np.isposinf(lp_hist[:, -1]).sum()), captured_at_start=int(np.isposinf(ref["logp0"]).sum()))
