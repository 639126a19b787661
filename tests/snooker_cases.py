"""The worlds tests/test_gpu_snooker.py runs against tests/snooker_reference.py, and what the reference alone must show of each
(tests/test_snooker_cases.py) for the bit comparison to be worth making.

Every world: N = 70 chains (one full wave and a part-filled one), G = 40 generations, an archive of N + 40 rows whose last N are
the chains' starting states (so 40 rows are archive-only), K in {3, 10}, snooker generations every 1, 3 or K generations.  The
populations start overdispersed about their targets, not at standard normals: a snooker step is accepted or rejected by its
log-density difference and its Jacobian together, and far out in a tail almost every step goes one way.

  * every world's reference shows at least one accepted and one rejected snooker step;
  * the worlds marked needs_invalid show steps whose |x - a|^2 or |x' - a|^2 is no positive normal double: chains started ON the
    rows of a small archive meet their own row as the anchor (e2 == 0), and an archive with +-inf coordinates gives infinite and
    NaN norms;
  * the tempered world has T = 0 at snooker generations and at ordinary ones."""
import zlib

import numpy as np

import demc_jl_amd as demc
import snooker_reference as sr
from program_texts import ROSENBROCK, box_closure, box_program, rosenbrock_closure

N, G = 70, 40
GAMMA_S = (1.2, 2.2)
LR_NOBS = 40


def _seed(name):
    return 20261020 + zlib.crc32(name.encode()) % 100000


def _problem(kind, d, name, m_arch=40):
    """target / closure, Z0 (m_arch archive-only rows, then the N starting states), eps, gamma"""
    r = np.random.default_rng(_seed(name))
    M0 = m_arch + N
    nrm = r.standard_normal((M0, d))
    if kind == "mvn":
        w = demc.workloads.mvnormal_problem(d, N)
        Z0 = w["mu"] + 2.0 * nrm @ np.linalg.cholesky(w["Sigma"]).T
        return dict(target=w["target"], closure=None, Z0=Z0, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "iso":
        w = demc.workloads.iso_quad_problem(d, N)
        return dict(target=w["target"], closure=None, Z0=w["mu"] + nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "lr":
        w = demc.workloads.linreg_problem(d, N, nobs=LR_NOBS)
        return dict(target=w["target"], closure=None, Z0=w["beta"] + 0.3 * nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "rosenbrock":
        return dict(target=demc.ProgramTarget(ROSENBROCK, d), closure=rosenbrock_closure, Z0=0.5 * nrm + 0.5, eps=1e-3 * np.ones(d), gamma=0.5)
    if kind == "box":               # bounded support: -inf outside |x_i| <= 1.5
        c, h = np.zeros(d), 1.5 * np.ones(d)
        return dict(target=box_program(c, h), closure=box_closure(c, h), Z0=0.8 * nrm, eps=1e-3 * np.ones(d), gamma=1.0)
    raise ValueError(kind)


def temperatures():
    """hot, cold, zero, huge, tiny in turn: with snooker generations every 3 each of them meets snooker and ordinary generations"""
    return np.array([(10.0, 0.25, 0.0, 1e300, 1e-300)[g % 5] for g in range(G)])


#        name               kind          d   K  every  more
WORLDS = {
    "mvn2":           ("mvn", 2, 3, 3, {}),
    "mvn5":           ("mvn", 5, 10, 10, {}),
    "mvn5_all":       ("mvn", 5, 3, 1, {}),                       # every generation of a whole run is a snooker generation
    "mvn7":           ("mvn", 7, 10, 3, {}),
    "mvn20":          ("mvn", 20, 3, 3, {}),
    "mvn33":          ("mvn", 33, 10, 1, {}),
    "iso10":          ("iso", 10, 10, 3, {}),
    "iso6":           ("iso", 6, 3, 1, {}),
    "lr10":           ("lr", 10, 3, 3, {}),
    "lr4":            ("lr", 4, 10, 10, {}),
    "rosenbrock7":    ("rosenbrock", 7, 10, 3, {}),
    "box4":           ("box", 4, 3, 3, {}),
    "mvn6_blocks":    ("mvn", 6, 10, 3, dict(blocks=[[0, 1], [2, 3], [4, 5]])),
    "mvn5_tempered":  ("mvn", 5, 10, 3, dict(tempered=True)),
    "mvn5_own_row":   ("mvn", 5, 10, 1, dict(m_arch=3, needs_invalid=True)),
    "iso6_inf":       ("iso", 6, 3, 3, dict(inf_rows=True, needs_invalid=True)),
}


def world(name):
    kind, d, K, every, more = WORLDS[name]
    p = _problem(kind, d, name, more.get("m_arch", 40))
    Z0 = np.array(p["Z0"], order="F")
    if more.get("inf_rows"):
        Z0[3, 1], Z0[11, 4], Z0[17, 0] = np.inf, -np.inf, np.inf       # archive-only rows
    return dict(name=name, kind=kind, d=d, N=N, G=G, K=K, every=every, gamma_s=GAMMA_S, seed=_seed(name), Z0=Z0,
                blocks=more.get("blocks", [list(range(d))]), temperature=temperatures() if more.get("tempered") else None,
                needs_invalid=bool(more.get("needs_invalid")), target=p["target"], closure=p["closure"], eps=p["eps"], gamma=p["gamma"])


def mixed_run(O, w, **over):
    """A MixedRun of the world, its options overridden by `over`."""
    kw = dict(N=w["N"], d=w["d"], K=w["K"], G=w["G"], blocks=w["blocks"], eps=w["eps"], seed=w["seed"], Z0=w["Z0"],
              target=None if w["closure"] else w["target"], closure=w["closure"], every=w["every"], gamma_s=w["gamma_s"])
    kw.update(over)
    return sr.MixedRun(O, **kw)


_REF = {}


def reference(O, name):
    """(world, the reference's result, its MixedRun) of the whole run in one piece; computed once and shared -- do not write to it."""
    if name not in _REF:
        w = world(name)
        run = mixed_run(O, w)
        run.run(1, w["G"], w["gamma"], w["temperature"])
        _REF[name] = (w, run.result(), run)
    return _REF[name]
