"""The worlds tests/test_gpu_crossover_adapt.py and tests/test_gpu_crossover_adapt_forms.py run against
tests/crossover_adapt_reference.py, and what the reference alone must show of them (tests/test_crossover_adapt_cases.py) for the
bit comparison to be worth making.

Every world has N not a multiple of 64 and more than one workgroup (a part-filled wave and the sum over the workgroups' slots).
WORLDS are the main ones: N = 100, a hundred and more generations, so that several updates are made and the weights move.
FORM_WORLDS are short (30 generations, updates behind 7, 14 and 21) and go through every ADAPT instantiation."""
import numpy as np

import crossover_adapt_reference as ar
import crossover_cases as cc
import crossover_reference as cr

N = 100
_T = dict(tempered=True)
#        name              kind    d   more
WORLDS = {
    "mvn5":           ("mvn", 5, dict(G=120, K=7, every=20, until=100)),                         # every coprime to K
    "mvn64_floor":    ("mvn", 64, dict(G=100, K=10, every=20, until=80, min_weight=8192)),        # the run-time-d form; every a multiple of K
    "mvn5_far":       ("mvn", 5, dict(G=100, K=10, every=25, until=100, far=True)),              # a tight start far out: clamped steps
    "iso10_const":    ("iso", 10, dict(G=100, K=10, every=25, until=75, const_col=3, N=70)),     # a constant column in the first period
    "mvn5_tempered":  ("mvn", 5, dict(G=100, K=10, every=20, until=100, N=130, **_T)),
    "mvn5_snooker":   ("mvn", 5, dict(G=100, K=10, every=20, until=80, snooker=4)),              # snooker generations on update positions
}
_F = dict(G=30, K=5, every=7, until=21, N=70)
FORM_WORLDS = {
    **{f"mvn{d}": ("mvn", d, _F) for d in (2, 3, 4, 8, 10, 20)},
    "iso10": ("iso", 10, _F), "lr10": ("lr", 10, _F), "lr26": ("lr", 26, _F),
    "mvn7": ("mvn", 7, _F), "iso4": ("iso", 4, _F), "lr9": ("lr", 9, _F),
    "mvn33": ("mvn", 33, _F), "mvn64": ("mvn", 64, _F), "iso64": ("iso", 64, _F), "lr64": ("lr", 64, dict(_F, nobs=70)),
    "prog_mvn2": ("prog_mvn", 2, _F), "rosenbrock7": ("rosenbrock", 7, _F), "prog_mvn32": ("prog_mvn", 32, _F),
    "mvn20_tempered": ("mvn", 20, dict(_F, **_T)), "mvn7_tempered": ("mvn", 7, dict(_F, **_T)), "lr10_tempered": ("lr", 10, dict(_F, **_T)),
    "rosenbrock7_tempered": ("rosenbrock", 7, dict(_F, **_T)),
}
ALL = {**WORLDS, **FORM_WORLDS}


def planned_kernel(w):
    """The name demcz_debug_kernel_name gives behind a crossover launch of an adapting handle."""
    plain = cc.planned_kernel(w)
    return plain.replace(">", ", adapt>", 1)


def world(name):
    kind, d, more = ALL[name]
    n = more.get("N", N)
    seed_name = "adapt_" + name
    if kind == "lr" and "nobs" in more:
        r = np.random.default_rng(cc._seed(seed_name))
        lw = cc.demc.workloads.linreg_problem(d, n, nobs=more["nobs"])
        p = dict(target=lw["target"], closure=None, Z0=lw["beta"] + 0.15 * r.standard_normal((40 + n, d)), eps=lw["eps_scale"], gamma=lw["gamma"])
    else:
        p = cc._problem(kind, d, seed_name, 40, n, 1.0)
    Z0 = np.array(p["Z0"], order="F")
    M0 = Z0.shape[0]
    if more.get("far"):
        # the chains start in one tight cluster six units out along every axis: their spread is tiny against the archive's
        # differences, so the first period's accepted steps are hundreds of standard deviations long
        r = np.random.default_rng(cc._seed(seed_name) + 1)
        Z0[M0 - n:] = Z0[M0 - n:].mean(axis=0) + 6.0 + 1e-3 * r.standard_normal((n, d))
    if "const_col" in more:
        Z0[M0 - n:, more["const_col"]] = 0.25
    g_total = more["G"]
    return dict(name=name, kind=kind, d=d, N=n, G=g_total, K=more["K"], ncr=3, delta_max=3, weights=None, every=more.get("snooker", 0),
                gamma_s=(1.2, 2.2), seed=cc._seed(seed_name), Z0=Z0, temperature=cc.temperatures(g_total) if more.get("tempered") else None,
                target=p["target"], ref_target=p.get("ref_target", p["target"]), closure=p["closure"], eps=p["eps"], gamma=p["gamma"],
                adapt_every=more["every"], adapt_until=more["until"], min_weight=more.get("min_weight", 656))


def adapt_run(O, w, **over):
    kw = dict(N=w["N"], d=w["d"], K=w["K"], G=w["G"], eps=w["eps"], seed=w["seed"], Z0=w["Z0"],
              target=None if w["closure"] else w["ref_target"], closure=w["closure"], ncr=w["ncr"], delta_max=w["delta_max"],
              weights=w["weights"], every=w["every"], gamma_s=w["gamma_s"], adapt_every=w["adapt_every"], adapt_until=w["adapt_until"],
              min_weight=w["min_weight"])
    kw.update(over)
    return ar.AdaptRun(O, **kw)


_REF = {}


def reference(O, name):
    """(world, the reference's result, its AdaptRun) of the whole run; computed once and shared -- do not write to it."""
    if name not in _REF:
        w = world(name)
        run = adapt_run(O, w)
        run.run(1, w["G"], w["gamma"], w["temperature"])
        _REF[name] = (w, run.result(), run)
    return _REF[name]


def lagged_reference(O, name, E):
    """The world under demcz_set_append_lag(E), as crossover_cases.lagged_reference makes it: the rows of boundary j join batch
    J = ceil(j / E) E and are drawn from generation (J + E) K + 1 on; the adaptation goes by positions and knows nothing of it."""
    key = (name, E)
    if key not in _REF:
        w = world(name)
        run = adapt_run(O, w, external=True)
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


def uneven_cuts(w):
    """The last generation of every call of a run cut unevenly: cuts on, one before and one behind the first update position, on
    and beside a K boundary, one call over several periods."""
    e, k = w["adapt_every"], w["K"]
    return sorted(({1, e - 1, e, e + 1, k, k + 1, 2 * e + 3, w["adapt_until"]} & set(range(1, w["G"]))) | {w["G"]})


# ---- what the reference shows of a world (tests/test_crossover_adapt_cases.py asserts on these) ----------------------------------------
def changed_updates(run):
    return sum(old != new for _, old, new, _ in run.update_log)


def redrawn_classes(O, run):
    """crossover steps whose class differs from the one the INITIAL weights would have drawn from the same word"""
    cum0 = cr.cumulative([1] * run.ncr if run.update_log == [] else run.update_log[0][1])
    n = 0
    for g, c, f in run.steps:
        r1, _ = O.draw_block(run.seed, run.chain_id0 + c, (g + run.rng_offset - 1) * run.S)
        n += cr.cr_class(cr.words(r1, 0)[1], cum0) != f["m"]
    return n


def clamped_steps(run):
    return sum(J >= ar.Q_ONE for _, _, _, J, _ in run.jumps)


def zero_q_steps(run):
    return sum(q == 0 for _, _, _, _, q in run.jumps)
