"""GPU: every instantiation of the crossover kernels, bit for bit against tests/crossover_reference.py.

tests/test_gpu_crossover.py runs the worlds of the feature's first tests; this file reaches the rest of what is compiled
(tests/crossover_cases.py: FORM_WORLDS) -- the specialised dimensions MvNormal 3, 4, 8, 10 and regression 26, the run-time-d form
of all three targets at d = 64, where the subset mask's bit 63 is used, the program units of d = 2, 3, 4 and 32, and tempered
runs of every kernel family -- and drives every world through calls that begin on, end on, stop short of and start behind a
K boundary, with calls of one generation on and off a boundary.  The name behind every call is held to the planned instantiation.
With an append lag on a one-rank communicator a launch spans K boundaries and stores the boundary snapshots itself.
No tolerance anywhere."""
import numpy as np
import pytest

import crossover_cases as cc
from helpers import same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")
# the last generation of every call (K = 5): 1 | 2-4 | 5 | 6-10 | 11-12 | 13 | 14-15 | 16-38 | 39-40
#   one generation off a boundary; up to the generation in front of one; one generation that is a boundary; a whole K-window;
#   a piece that starts behind a boundary; one generation in mid-window; a piece that ends on a boundary; several windows; the rest
CALLS = [1, 4, 5, 10, 12, 13, 15, 38, 40]


def _run(demc, w, comm=False, lag=0):
    M0 = w["Z0"].shape[0]
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (w["G"] // w["K"] + 1), Gcap=w["G"], blockindex=[range(w["d"])],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
        if comm:
            e.comm_init(e.comm_unique_id(), 1, 0)
        if lag:
            e.set_append_lag(lag)
        e.set_crossover(w["ncr"], w["delta_max"], w["weights"])
        names, launches = [], []
        a = 1
        for b in ([w["G"]] if lag else CALLS):
            e.run(a, b, w["gamma"], None if w["temperature"] is None else w["temperature"][a - 1:b])
            names.append(e.kernel_name())
            launches.append(e.info()["window_launches"])
            a = b + 1
        e.synchronize()
        chain, lobj = e.get_history(1, w["G"])
        X, lp, Z, M = e.get_state()
        return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=e.get_changed(1, w["G"]),
                    crossover=e.crossover, names=names, launches=launches)
    finally:
        e.close()


def _same(got, ref, run, what):
    same_bits(got, ref, keys=KEYS, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"
    tried, accepted = run.counts()
    assert np.array_equal(got["crossover"].tried, tried) and np.array_equal(got["crossover"].accepted, accepted), what


@pytest.mark.parametrize("name", [n for n in cc.ALL if cc.ALL[n][3].get("N", cc.N) == cc.N and not cc.ALL[n][3].get("every")])
def test_every_instantiation_through_calls_about_the_k_boundary(demc, oracle, name):
    w, ref, run = cc.reference(oracle, name)
    got = _run(demc, w)
    _same(got, ref, run, name)
    assert got["names"] == [cc.planned_kernel(w)] * len(CALLS), name
    # a launch ends at its call's end and at the next multiple of K: 1 | 2-4 | 5 | 6-10 | 11-12 | 13 | 14-15 | 16-20 ... 36-38 | 39-40
    assert got["launches"] == [1, 2, 3, 4, 5, 6, 7, 12, 13], name


def test_the_worlds_launch_every_planned_kernel():
    names = [n for n in cc.ALL if cc.ALL[n][3].get("N", cc.N) == cc.N and not cc.ALL[n][3].get("every")]
    assert {cc.planned_kernel(cc.world(n)) for n in names} == cc.PLANNED_NAMES


@pytest.mark.parametrize("name,E", [("mvn5", 2), ("mvn33", 3), ("rosenbrock7", 2), ("mvn20_tempered", 3)])
def test_a_launch_that_spans_k_boundaries(demc, oracle, name, E):
    """A one-rank communicator with an append lag: one launch covers a batch of K-windows, counts its boundaries down itself and
    stores each boundary's states into the snapshot buffer the all-gather sends from."""
    w, ref, run = cc.lagged_reference(oracle, name, E)
    got = _run(demc, w, comm=True, lag=E)
    _same(got, ref, run, f"{name} lag {E}")
    assert got["names"] == [cc.planned_kernel(w)]
    assert got["launches"][-1] < w["G"] // w["K"], f"{name}: {got['launches']} launches: none spans a K boundary"
    _, plain, _ = cc.reference(oracle, name)
    assert not np.array_equal(ref["chain"], plain["chain"])           # the lag shows in the run
