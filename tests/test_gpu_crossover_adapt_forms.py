"""GPU: every ADAPT instantiation of the crossover kernels, bit for bit against tests/crossover_adapt_reference.py.

tests/crossover_adapt_cases.py: FORM_WORLDS -- the ten specialised kernels (MvNormal 2, 3, 4, 8, 10, 20 here and 5 in
tests/test_gpu_crossover_adapt.py; iso-quad 10; regression 10, 26), the run-time-d form of all three targets, at d = 33 and 64 too,
the program units of d = 2, 7 and 32, and a tempered run of every family.  N = 70, K = 5, 30 generations, updates behind 7, 14 and
21.  Every world is driven through calls that begin on, end on, stop short of and start behind an update position and a K boundary;
the kernel name and the launch count behind every call show the planner's cuts.  With an append lag a launch that would span an
update position is cut there.  No tolerance anywhere."""
import numpy as np
import pytest

import crossover_adapt_cases as ac
from helpers import same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")
# the last generation of every call (K = 5, updates behind 7, 14, 21):
#   1 | 2-4 | 5 | 6 | 7 | 8-10 | 11-13 | 14 | 15 | 16-22 | 23-30
#   one generation; up to the one in front of a K boundary; a boundary alone; the generation in front of an update; the update's
#   generation alone; a piece that starts behind an update and ends on a boundary; one that stops short of an update; an update alone
#   behind a cut; a boundary behind an update; a piece over a boundary, the last update and one generation more; the rest
CALLS = [1, 4, 5, 6, 7, 10, 13, 14, 15, 22, 30]
# launches end at a call's end, a multiple of K and -- up to 21 -- a multiple of 7: 16-20 | 21 | 22 and 23-25 | 26-30
LAUNCHES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14]
UPDATES = [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3]


def _run(demc, w, lag=0):
    M0 = w["Z0"].shape[0]
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (w["G"] // w["K"] + 1), Gcap=w["G"], blockindex=[range(w["d"])],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
        if lag:
            e.set_append_lag(lag)
        e.set_crossover(w["ncr"], w["delta_max"], w["weights"])
        e.set_crossover_adapt(w["adapt_every"], w["adapt_until"], w["min_weight"])
        names, launches, updates = [], [], []
        a = 1
        for b in ([w["G"]] if lag else CALLS):
            e.run(a, b, w["gamma"], None if w["temperature"] is None else w["temperature"][a - 1:b])
            names.append(e.kernel_name())
            launches.append(e.info()["window_launches"])
            updates.append(e.crossover_adapt.updates)
            a = b + 1
        e.synchronize()
        chain, lobj = e.get_history(1, w["G"])
        X, lp, Z, M = e.get_state()
        return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=e.get_changed(1, w["G"]),
                    crossover=e.crossover, adapt=e.crossover_adapt, names=names, launches=launches, updates=updates)
    finally:
        e.close()


def _same(got, ref, run, what):
    same_bits(got, ref, keys=KEYS, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"
    a, st = got["adapt"], run.state()
    assert (list(a.weights), list(a.dist), list(a.tried), a.updates) == (st["weights"], st["dist"], st["tried"], st["updates"]), \
        f"{what}: {a} / {st}"
    same_bits(dict(rsd=a.rsd), dict(rsd=np.array(st["rsd"])), keys=("rsd",), what=what)
    tried, accepted = run.counts()
    assert np.array_equal(got["crossover"].tried, tried) and np.array_equal(got["crossover"].accepted, accepted), what


@pytest.mark.parametrize("name", list(ac.FORM_WORLDS))
def test_every_instantiation_through_calls_about_updates_and_k_boundaries(demc, oracle, name):
    w, ref, run = ac.reference(oracle, name)
    got = _run(demc, w)
    _same(got, ref, run, name)
    assert got["names"] == [ac.planned_kernel(w)] * len(CALLS), name
    assert got["launches"] == LAUNCHES, name
    assert got["updates"] == UPDATES, name


def test_the_worlds_launch_every_adapt_kernel():
    import crossover_cases as cc
    names = {ac.planned_kernel(ac.world(n)) for n in ac.ALL}
    want = ({f"demcz::window_kernel_cr<{cc.TARGET_NAME[k]}, {d}, adapt>" for k, ds in cc.SPECIALISED.items() for d in ds}
            | {f"demcz::window_kernel_cr_generic<{t}, adapt>" for t in cc.TARGET_NAME.values()}
            | {f"demcz::window_kernel_cr<4, {d}, adapt> (program)" for d in (2, 7, 32)})
    assert names == want
    generic_d = {(ac.ALL[n][0], ac.ALL[n][1]) for n in ac.ALL if "generic" in ac.planned_kernel(ac.world(n))}
    assert {("mvn", 33), ("mvn", 64), ("iso", 64), ("lr", 64)} <= generic_d


@pytest.mark.parametrize("name,E", [("mvn10", 2), ("mvn7", 3)])
def test_a_launch_that_would_span_an_update_is_cut_there(demc, oracle, name, E):
    """With an append lag one launch covers a batch of E K-windows -- and ends at the update position inside it."""
    w, ref, run = ac.lagged_reference(oracle, name, E)
    got = _run(demc, w, lag=E)
    _same(got, ref, run, f"{name} lag {E}")
    assert got["names"] == [ac.planned_kernel(w)]
    # E = 2: 1-7 | 8-10 | 11-14 | 15-20 | 21 | 22-30.  E = 3: 1-7 | 8-14 | 15 | 16-21 | 22-30
    assert got["launches"] == [6 if E == 2 else 5], name
    _, plain, _ = ac.reference(oracle, name)
    assert not np.array_equal(ref["chain"], plain["chain"])           # the lag shows in the run
