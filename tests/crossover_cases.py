"""The worlds tests/test_gpu_crossover.py and tests/test_gpu_crossover_forms.py run against tests/crossover_reference.py, and what
the reference alone must show of each (tests/test_crossover_cases.py) for the bit comparison to be worth making.

A main world: N = 70 chains (one full wave and a part-filled one), G = 40 generations, K = 5, an archive of 40 archive-only rows
and the chains' starting states, drawn from the target's neighbourhood (a crossover step is accepted about one time in four
there; far out in a tail almost every step goes one way).  Every generation that is not a snooker generation is a crossover
generation.

WORLDS are the worlds of tests/test_gpu_crossover.py; FORM_WORLDS add what they leave out of the instantiations (the specialised
dimensions 3, 4, 8, 10 and regression 26, the run-time-d form at d = 64 where the mask's bit 63 is used, the program units of
d = 2, 3, 4, 32, tempered forms of every family).

What tests/test_crossover_cases.py asks (from the reference alone):
  * in every world with ncr = 3, delta_max = 3 each of the nine (class, delta) cells has at least 10 accepted and at least 10
    rejected steps;
  * in worlds with d <= 5 at least 10 fallback steps (nothing selected, p* alone moves), accepted and rejected ones among them;
  * in every tempered world at least 10 steps whose outcome differs from the untempered comparison of the same step;
  * the per-class tried counts add up to chains x crossover generations."""
import zlib

import numpy as np

import crossover_reference as cr
import demc_jl_amd as demc
from program_texts import ROSENBROCK, box_closure, box_program, mvn_program, rosenbrock_closure

N, G, K = 70, 40, 5
LR_NOBS = 40


def _seed(name):
    return 20261021 + zlib.crc32(name.encode()) % 100000


def _problem(kind, d, name, m_arch, n, spread):
    r = np.random.default_rng(_seed(name))
    M0 = m_arch + n
    nrm = r.standard_normal((M0, d))
    if kind in ("mvn", "prog_mvn"):
        w = demc.workloads.mvnormal_problem(d, n)
        Z0 = w["mu"] + spread * nrm @ np.linalg.cholesky(w["Sigma"]).T
        t = w["target"]
        if kind == "prog_mvn":      # the device runs the program, the reference the oracle's built-in log-density
            return dict(target=mvn_program(t.mu, t.W, t.c0), ref_target=t, closure=None, Z0=Z0, eps=w["eps_scale"], gamma=w["gamma"])
        return dict(target=t, closure=None, Z0=Z0, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "iso":
        w = demc.workloads.iso_quad_problem(d, n)
        return dict(target=w["target"], closure=None, Z0=w["mu"] + (0.7 * spread) * nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "lr":
        w = demc.workloads.linreg_problem(d, n, nobs=LR_NOBS)
        return dict(target=w["target"], closure=None, Z0=w["beta"] + (0.15 * spread) * nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "rosenbrock":
        return dict(target=demc.ProgramTarget(ROSENBROCK, d), closure=rosenbrock_closure, Z0=(0.25 * spread) * nrm + 0.5, eps=1e-3 * np.ones(d), gamma=0.5)
    if kind == "box":               # bounded support: -inf outside |x_i| <= 1.5
        c, h = np.zeros(d), 1.5 * np.ones(d)
        return dict(target=box_program(c, h), closure=box_closure(c, h), Z0=0.8 * nrm, eps=1e-3 * np.ones(d), gamma=1.0)
    raise ValueError(kind)


def temperatures(g_total):
    """hot, cold, zero, huge, tiny in turn"""
    return np.array([(10.0, 0.25, 0.0, 1e300, 1e-300)[g % 5] for g in range(g_total)])


_T = dict(tempered=True)
#        name               kind          d   (ncr, delta_max)  more
WORLDS = {
    "mvn2":           ("mvn", 2, (3, 3), {}),                      # the specialised target classes
    "mvn5":           ("mvn", 5, (3, 3), {}),
    "mvn20":          ("mvn", 20, (3, 3), {}),
    "iso10":          ("iso", 10, (3, 3), {}),
    "lr10":           ("lr", 10, (3, 3), {}),
    "iso4":           ("iso", 4, (3, 3), {}),                      # the run-time-d form
    "mvn7":           ("mvn", 7, (3, 3), {}),
    "lr9":            ("lr", 9, (3, 3), {}),
    "mvn33":          ("mvn", 33, (3, 3), {}),                     # a second word of the mask
    "rosenbrock7":    ("rosenbrock", 7, (3, 3), {}),
    "box4":           ("box", 4, (3, 3), dict(inf_rows=True)),     # -inf outside the box, +-inf in archive-only rows
    "mvn5_one_class": ("mvn", 5, (1, 1), {}),                      # every parameter, one pair: the full-block move but for its stream
    "mvn7_eight":     ("mvn", 7, (8, 2), {}),
    "mvn5_zero_weight": ("mvn", 5, (3, 3), dict(weights=[2, 0, 5])),
    "mvn7_zero_first": ("mvn", 7, (4, 2), dict(weights=[0, 3, 0, 1])),
    "mvn5_tempered":  ("mvn", 5, (3, 3), _T),
    "mvn7_tempered":  ("mvn", 7, (3, 3), _T),
    "mvn5_snooker":   ("mvn", 5, (3, 3), dict(every=4)),
    "mvn7_snooker":   ("mvn", 7, (3, 3), dict(every=4)),
    "mvn5_two_rows_k1": ("mvn", 5, (2, 2), dict(N=2, m_arch=0, K=1)),      # M0 = 2: the rows of the first generation are forced
    "mvn5_n1":        ("mvn", 5, (2, 2), dict(N=1)),
    "mvn7_n64":       ("mvn", 7, (3, 3), dict(N=64)),
}
FORM_WORLDS = {
    "mvn3":           ("mvn", 3, (3, 3), {}),
    "mvn4":           ("mvn", 4, (3, 3), {}),
    "mvn8":           ("mvn", 8, (3, 3), {}),
    "mvn10":          ("mvn", 10, (3, 3), {}),
    "lr26":           ("lr", 26, (3, 3), {}),
    "mvn64":          ("mvn", 64, (3, 3), {}),                     # MAX_D: the mask's bit 63
    "iso64":          ("iso", 64, (3, 2), {}),
    "lr64":           ("lr", 64, (3, 2), dict(nobs=70)),
    "prog_mvn2":      ("prog_mvn", 2, (3, 3), {}),
    "prog_mvn3":      ("prog_mvn", 3, (3, 3), {}),
    "prog_mvn4":      ("prog_mvn", 4, (3, 3), {}),
    "prog_mvn32":     ("prog_mvn", 32, (3, 3), {}),
    "mvn20_tempered": ("mvn", 20, (3, 3), _T),
    "iso10_tempered": ("iso", 10, (3, 3), _T),
    "lr10_tempered":  ("lr", 10, (3, 3), _T),
    "lr9_tempered":   ("lr", 9, (3, 3), _T),
    "iso4_tempered":  ("iso", 4, (3, 3), _T),
    "rosenbrock7_tempered": ("rosenbrock", 7, (3, 3), _T),
}
ALL = {**WORLDS, **FORM_WORLDS}

# the d each built-in target's one-lane dispatch specialises (crossover_kernel_fn); every other d <= 64 runs the run-time-d form
SPECIALISED = {"mvn": (2, 3, 4, 5, 8, 10, 20), "iso": (10,), "lr": (10, 26)}
TARGET_NAME = {"mvn": "MVNORMAL", "iso": "ISO_QUAD", "lr": "LINREG_SSE"}
PLANNED_NAMES = (
    {f"demcz::window_kernel_cr<{TARGET_NAME[k]}, {d}>" for k, ds in SPECIALISED.items() for d in ds}
    | {f"demcz::window_kernel_cr_generic<{t}>" for t in TARGET_NAME.values()}
    | {f"demcz::window_kernel_cr<4, {d}> (program)" for d in (2, 3, 4, 7, 32)})


def planned_kernel(w):
    """The name demcz_debug_kernel_name gives behind a crossover launch of the world."""
    kind, d = w["kind"], w["d"]
    if kind not in SPECIALISED:
        return f"demcz::window_kernel_cr<4, {d}> (program)"
    return f"demcz::window_kernel_cr<{TARGET_NAME[kind]}, {d}>" if d in SPECIALISED[kind] else f"demcz::window_kernel_cr_generic<{TARGET_NAME[kind]}>"


def world(name):
    kind, d, (ncr, delta_max), more = ALL[name]
    n = more.get("N", N)
    if kind == "lr" and "nobs" in more:
        r = np.random.default_rng(_seed(name))
        w = demc.workloads.linreg_problem(d, n, nobs=more["nobs"])
        p = dict(target=w["target"], closure=None, Z0=w["beta"] + 0.15 * r.standard_normal((40 + n, d)), eps=w["eps_scale"], gamma=w["gamma"])
    else:
        p = _problem(kind, d, name, more.get("m_arch", 40), n, more.get("spread", 1.0))
    Z0 = np.array(p["Z0"], order="F")
    if more.get("inf_rows"):
        Z0[3, 1], Z0[11, 2], Z0[17, 0] = np.inf, -np.inf, np.inf       # archive-only rows
    g_total = more.get("G", G)
    return dict(name=name, kind=kind, d=d, N=n, G=g_total, K=more.get("K", K), ncr=ncr, delta_max=delta_max, weights=more.get("weights"),
                every=more.get("every", 0), gamma_s=(1.2, 2.2), seed=_seed(name), Z0=Z0,
                temperature=temperatures(g_total) if more.get("tempered") else None, target=p["target"],
                ref_target=p.get("ref_target", p["target"]), closure=p["closure"], eps=p["eps"], gamma=p["gamma"])


def uneven_cuts(w):
    """The last generation of every call of a run cut unevenly: a one-generation call, calls that end in front of, on and behind a
    K boundary, a call over several K-windows."""
    return sorted({1, 4, 5, 11, 12, 30, w["G"]} & set(range(1, w["G"] + 1)) | {w["G"]})


def crossover_run(O, w, **over):
    kw = dict(N=w["N"], d=w["d"], K=w["K"], G=w["G"], eps=w["eps"], seed=w["seed"], Z0=w["Z0"],
              target=None if w["closure"] else w["ref_target"], closure=w["closure"], ncr=w["ncr"], delta_max=w["delta_max"],
              weights=w["weights"], every=w["every"], gamma_s=w["gamma_s"])
    kw.update(over)
    return cr.CrossoverRun(O, **kw)


_REF = {}


def reference(O, name):
    """(world, the reference's result, its CrossoverRun) of the whole run; computed once and shared -- do not write to it."""
    if name not in _REF:
        w = world(name)
        run = crossover_run(O, w)
        run.run(1, w["G"], w["gamma"], w["temperature"])
        _REF[name] = (w, run.result(), run)
    return _REF[name]


def lagged_reference(O, name, E):
    """The world under demcz_set_append_lag(E): the rows of boundary j join batch J = ceil(j / E) E and are drawn from generation
    (J + E) K + 1 on; at the end of the run all of them are in the archive, in the order of their boundaries."""
    key = (name, E)
    if key not in _REF:
        w = world(name)
        run = crossover_run(O, w, external=True)
        Kw, pending = w["K"], []
        for a in range(1, w["G"] + 1, Kw):
            b = min(a + Kw - 1, w["G"])
            while pending and pending[0][0] <= a:
                run.append_rows(pending.pop(0)[1])
            run.run(a, b, w["gamma"], None if w["temperature"] is None else w["temperature"][a - 1:b])
            if b % Kw == 0:
                J = -(-(b // Kw) // E) * E
                pending.append(((J + E) * Kw + 1, run.result()["X"]))
        for _, rows in pending:
            run.append_rows(rows)
        _REF[key] = (w, run.result(), run)
    return _REF[key]


# ---- what the reference shows of a world (tests/test_crossover_cases.py asserts on these) -------------------------------------------------
def cell_counts(run):
    """{(class, delta): [accepted, rejected]} over the crossover steps"""
    out = {}
    for _, _, f in run.steps:
        c = out.setdefault((f["m"], f["delta"]), [0, 0])
        c[0 if f["accepted"] else 1] += 1
    return out


def fallback_counts(run):
    """(accepted, rejected) fallback steps"""
    fb = [f for _, _, f in run.steps if f["fallback"]]
    return sum(f["accepted"] for f in fb), sum(not f["accepted"] for f in fb)


def tempered_flips(run):
    return sum(f["accepted"] != f["accepted_untempered"] for _, _, f in run.steps)
