"""GPU: every snooker kernel instantiation, form and step outcome, bit for bit against tests/snooker_reference.py.

tests/snooker_cases.py holds the worlds, tests/test_snooker_cases.py holds them to their conditions by the reference alone: in every
main world steps exist that a kernel with the Jacobian's exponent one off, the temperature ignored or applied to the Jacobian, or a
blocked handle's quadratic form summed in one piece would decide otherwise.  One handle per world; its schedule of demcz_run calls
ends one call in front of a snooker generation and one on it, and the new tempered worlds run one piece without temperatures.
After every call the count of snooker launches and of window launches is held to the plan restated in the cases file, and behind a
call that ends on a snooker generation the kernel's reported name: the ten specialised built-in instantiations, the three
run-time-d ones and the program units of d = 2, 3, 4, 7, 32.  At the end chain, log_obj, X, logp, Z, M and the changed counts of
every generation are compared, and the ballots answer changed_total from generation 1 and from the last snooker generation.

The edge worlds run the same comparison: populations of 1, 2, 63, 64, 65 and 129 chains, archives of exactly three rows, K = 1,
snooker generations rarer than the run is long or one off the K-window, own-row anchors and +-inf rows through the scalar-register
whitening, gamma_lo == gamma_hi.  On top of them: a handle that keeps no history, streamed history, a one-rank communicator, and
the same with an append lag (the snooker kernel's store of the boundary snapshot into the all-gather's send buffer: the route
without a lag gathers from the state and hands the kernel no snapshot buffer).  No tolerance anywhere."""
import numpy as np
import pytest

import snooker_cases as sc
from helpers import same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")


def _run(demc, w, history=True, comm=False, lag=0, stream=False, snooker=True):
    """The world on one handle, call by call; what the handle reports behind every call, and its results."""
    M0 = w["Z0"].shape[0]
    G = w["G"]
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (G // w["K"] + 1), Gcap=G if history else 0, blockindex=w["blocks"],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], lanes_per_chain=1)
    try:
        if comm:
            e.comm_init(e.comm_unique_id(), 1, 0)
        if lag:
            e.set_append_lag(lag)
        e.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
        if stream:
            e.history_stream(True)
        if snooker:
            e.set_snooker(w["every"], w["gamma_s"])
        got = dict(snooker_launches=[], launches=[], names=[])
        for a, b, tempered in w["pieces"]:
            e.run(a, b, w["gamma"], sc.piece_temperature(w, a, b, tempered))
            got["snooker_launches"].append(e.snooker[3])
            got["launches"].append(e.info()["window_launches"])
            got["names"].append(e.kernel_name())
        X, lp, Z, M = e.get_state()
        got.update(X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, peer_status=e.peer_status())
        got["total"], got["from_ballots"] = e.changed_total(1, G, with_source=True)
        sn = sc.snooker_generations(w) if snooker else []
        if sn:
            got["tail"], got["tail_from_ballots"] = e.changed_total(sn[-1], G, with_source=True)
        if history:
            got["chain"], got["log_obj"] = e.get_history(1, G)
            got["changed"] = e.get_changed(1, G)
            if stream:
                got["streamed"] = e.take_history(1, G)
        return got
    finally:
        e.close()


def _held_to_the_plan(w, got, what):
    sn = sc.snooker_generations(w)
    ends = [b for _, b, _ in w["pieces"]]
    assert got["snooker_launches"] == [sum(g <= b for g in sn) for b in ends], f"{what}: snooker launches behind every call"
    assert got["launches"] == sc.launches_after(w), f"{what}: window launches behind every call"
    for b, name in zip(ends, got["names"]):
        if b in sn:
            assert name == sc.planned_kernel(w), f"{what}: the call that ends on snooker generation {b} ran {name}"
        else:
            assert "snooker" not in name, f"{what}: the call that ends on the ordinary generation {b} ran {name}"


def _same(got, ref, what, history=True):
    same_bits(got, ref, keys=KEYS if history else KEYS[2:], what=what)
    assert got["M"] == ref["M"], what
    assert (got["total"], got["from_ballots"]) == (int(ref["changed"].sum()), True), f"{what}: changed_total from the ballots"
    if history:
        assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"


def _world_is_the_reference(demc, oracle, name, **how):
    w, ref, run = sc.lagged_reference(oracle, name, how["lag"]) if how.get("lag") else sc.reference(oracle, name)
    got = _run(demc, w, **how)
    what = name + "".join(f", {k}" for k, v in how.items() if v) + (", no history" if how.get("history") is False else "")
    _held_to_the_plan(w, got, what)
    _same(got, ref, what, history=how.get("history", True))
    if run.snooker_generations:
        g = run.snooker_generations[-1]
        assert (got["tail"], got["tail_from_ballots"]) == (int(ref["changed"][g - 1:].sum()), True), f"{what}: changed_total from generation {g}"
    return w, ref, got


@pytest.mark.parametrize("name", list(sc.MAIN))
def test_every_main_world_is_the_reference_bit_for_bit(demc, oracle, name):
    _world_is_the_reference(demc, oracle, name)


def test_the_main_worlds_ran_every_planned_kernel():
    """(What the cases file plans is what the handles above were held to, call by call.)"""
    assert {sc.planned_kernel(sc.world(n)) for n in sc.MAIN} == sc.PLANNED_NAMES and len(sc.PLANNED_NAMES) == 18


@pytest.mark.parametrize("name", [n for n in sc.EDGE_WORLDS if n != "mvn5_never"])
def test_every_edge_world_is_the_reference_bit_for_bit(demc, oracle, name):
    _world_is_the_reference(demc, oracle, name)


def test_snooker_generations_rarer_than_the_run_is_long(demc, oracle):
    """every > G: no snooker launch, and the bits of the handle on which demcz_set_snooker was never called."""
    w, ref, got = _world_is_the_reference(demc, oracle, "mvn5_never")
    assert got["snooker_launches"][-1] == 0 and all("snooker" not in n for n in got["names"])
    plain = _run(demc, w, snooker=False)
    same_bits(plain, got, keys=KEYS, what="without set_snooker")
    assert plain["launches"] == got["launches"] and np.array_equal(plain["changed"], got["changed"])


@pytest.mark.parametrize("name", ["mvn8", "mvn7", "mvn8_n65", "mvn7_n65"])
def test_a_handle_without_history(demc, oracle, name):
    """Gcap = 0: P.chain is a null pointer in both kernels.  X, logp, Z, M and the ballots."""
    _world_is_the_reference(demc, oracle, name, history=False)


@pytest.mark.parametrize("name", ["mvn8", "mvn7"])
def test_streamed_history_is_copied_history_is_the_reference(demc, oracle, name):
    _, _, got = _world_is_the_reference(demc, oracle, name, stream=True)
    chain, log_obj = got["streamed"]
    same_bits(dict(chain=chain, log_obj=log_obj), got, keys=("chain", "log_obj"), what=f"{name}: streamed against copied")


@pytest.mark.parametrize("name", ["mvn5", "mvn7"])
def test_the_one_rank_communicator_route(demc, oracle, name):
    """demcz_comm_init with one rank: the rows of a K boundary are gathered from the state the snooker kernel left (in mvn5 every
    snooker generation is such a boundary).  A one-lane handle has no in-launch hand-off, so the communicator leaves it in peer
    mode 0 with no peers -- the mode demcz_set_snooker asks for."""
    _, _, got = _world_is_the_reference(demc, oracle, name, comm=True)
    assert got["peer_status"] == (0, 0)


@pytest.mark.parametrize("name,E", sc.LAGGED)
def test_the_one_rank_communicator_route_with_an_append_lag(demc, oracle, name, E):
    """Only a sharded handle with an append lag hands the kernels a snapshot buffer: at a K boundary the snooker kernel stores the
    chains' states into it (WindowParams::snap), the batched ncclAllGather on the side stream turns them into archive rows, and
    they are drawn from E batches later.  Every snooker generation of mvn5, every tenth of mvn33 (the run-time-d kernel) and
    every third of iso6 is such a boundary."""
    _, _, got = _world_is_the_reference(demc, oracle, name, comm=True, lag=E)
    assert got["peer_status"] == (0, 0)
