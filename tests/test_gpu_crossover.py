"""GPU: crossover generations (demcz_set_crossover, window_kernel_cr) bit for bit against tests/crossover_reference.py.

The worlds are tests/crossover_cases.py's (held to their conditions by the reference alone in tests/test_crossover_cases.py):
N = 70, 40 generations, K = 5; the specialised target classes and the run-time-d form, a program target, a program with bounded
support and +-inf in the archive, (ncr, delta_max) = (3, 3), (1, 1), (8, 2) and weights with zeros, temperatures with zeros,
snooker generations every 4, an archive of two rows with K = 1, populations of 1 and 64.  chain, log_obj, the final X and logp,
Z, M and the per-generation changed counts are compared without tolerance, tried / accepted per class for equality.  Every world
runs as one call, cut into uneven calls and through demcz_run_checked; then a checkpoint resume, two host-driven shards, every
refusal, and demcz_sample / demcz_anneal end to end."""
import ctypes as C

import numpy as np
import pytest

import crossover_cases as cc
from helpers import same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")


def _engine(demc, w, N=None, chain_id0=0, external=False, crossover=True, lanes=1):
    N = w["N"] if N is None else N
    M0 = w["Z0"].shape[0]
    e = demc.HipEngine(N=N, d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (w["G"] // w["K"] + 1), Gcap=w["G"], blockindex=[range(w["d"])],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], chain_id0=chain_id0, lanes_per_chain=lanes)
    X0 = w["Z0"][M0 - w["N"]:]
    e.set_state(X0[chain_id0:chain_id0 + N], None, w["Z0"])
    if external:
        e.set_external_append(True)
    if crossover:
        e.set_crossover(w["ncr"], w["delta_max"], w["weights"])
    if w["every"]:
        e.set_snooker(w["every"], w["gamma_s"])
    return e


def _collect(e, G):
    chain, lobj = e.get_history(1, G)
    X, lp, Z, M = e.get_state()
    return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=e.get_changed(1, G),
                crossover=e.crossover)


def _temps(w, a, b):
    return None if w["temperature"] is None else w["temperature"][a - 1:b]


def _run(demc, w, cuts=None, checked=0):
    """The world on one handle: demcz_run called once or piece by piece (cuts: the last generation of every piece), or
    demcz_run_checked with an R-hat slab of `checked` generations that never stops early."""
    e = _engine(demc, w)
    try:
        if checked:
            g_stop, mx, _ = e.run_checked(1, w["G"], w["gamma"], checked, threshold=0.0, temperature=_temps(w, 1, w["G"]))
            assert g_stop == w["G"] and len(mx) == w["G"] // checked
        else:
            a = 1
            for b in (cuts or [w["G"]]):
                e.run(a, b, w["gamma"], _temps(w, a, b))
                a = b + 1
        got = _collect(e, w["G"])
        got["total"], got["from_ballots"] = e.changed_total(1, w["G"], with_source=True)
        got["name"] = e.kernel_name()
        return got
    finally:
        e.close()


def _same(got, ref, run, what):
    same_bits(got, ref, keys=KEYS, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"
    if run is not None:
        tried, accepted = run.counts()
        c = got["crossover"]
        assert (c.ncr, c.delta_max, list(c.weights)) == (run.ncr, run.delta_max, run.weights), what
        assert np.array_equal(c.tried, tried) and np.array_equal(c.accepted, accepted), f"{what}: tried {c.tried} / {tried}, accepted {c.accepted} / {accepted}"


@pytest.mark.parametrize("name", list(cc.WORLDS))
def test_every_world_is_the_reference_bit_for_bit(demc, oracle, name):
    w, ref, run = cc.reference(oracle, name)
    got = _run(demc, w)
    _same(got, ref, run, name)
    assert (got["total"], got["from_ballots"]) == (int(ref["changed"].sum()), True), f"{name}: changed_total from the ballots"
    if not (w["every"] and w["G"] % w["every"] == 0):          # the last launch was a crossover launch
        assert got["name"] == cc.planned_kernel(w), name
    else:
        assert "snooker_kernel" in got["name"], name
    rate = got["crossover"].accept_rate
    tried, accepted = run.counts()
    assert all((np.isnan(rate[k]) and tried[k] == 0) or rate[k] == accepted[k] / tried[k] for k in range(w["ncr"]))


@pytest.mark.parametrize("name", list(cc.WORLDS))
def test_a_run_cut_into_uneven_calls_is_the_uncut_run(demc, oracle, name):
    w, ref, run = cc.reference(oracle, name)
    cuts = cc.uneven_cuts(w)
    _same(_run(demc, w, cuts), ref, run, f"{name} cut at {cuts}")


@pytest.mark.parametrize("name", list(cc.WORLDS))
def test_run_checked_is_the_run(demc, oracle, name):
    """demcz_run_checked goes through the same executor: two R-hat slabs of 20 generations."""
    w, ref, run = cc.reference(oracle, name)
    _same(_run(demc, w, checked=20), ref, run, f"{name} through run_checked")


def test_resume_through_a_checkpoint_is_the_uninterrupted_run(demc, oracle, tmp_path):
    """The first part's length is a multiple of K; crossover and snooker_every are passed again and the choices follow the streams."""
    w, ref, _ = cc.reference(oracle, "mvn7_snooker")
    kw = dict(verbose=False, seed=w["seed"], snooker_every=w["every"], snooker_gamma=w["gamma_s"], crossover=(w["ncr"], w["delta_max"]))
    args = (1, [range(w["d"])], w["eps"], w["gamma"])
    whole, Zw = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], 40, *args, **kw)
    first, Z1 = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], 15, *args, **kw)
    demc.save_checkpoint(tmp_path / "ck.npz", first, Z1, seed=w["seed"])
    prev, Zc, done, seed = demc.load_checkpoint(tmp_path / "ck.npz")
    assert done == 15
    kw["seed"] = seed
    second, Z2 = demc.demcz_sample(w["target"], Zc, w["N"], w["K"], 25, *args, prevrun=prev, **kw)
    assert np.array_equal(second.chain[:, :, 1:], whole.chain[:, :, 15:]) and np.array_equal(second.log_obj[:, 1:], whole.log_obj[:, 15:])
    assert np.array_equal(Z2, Zw) and np.array_equal(second.Xcurrent, whole.Xcurrent)
    assert np.array_equal(whole.chain, ref["chain"]) and np.array_equal(Zw, ref["Z"])


def test_resume_through_set_rng_offset_on_a_fresh_handle(demc, oracle):
    """set_crossover on the fresh handle, then set_rng_offset: generations 16..40 of the whole run."""
    w, ref, _ = cc.reference(oracle, "mvn5_snooker")
    first = cc.crossover_run(oracle, w)
    first.run(1, 15, w["gamma"])
    r1 = first.result()
    M0 = r1["M"]
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * 6, Gcap=25, blockindex=[range(w["d"])], eps_scale=w["eps"], seed=w["seed"],
                       target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(r1["X"], r1["logp"], r1["Z"])
        e.set_crossover(w["ncr"], w["delta_max"])
        e.set_rng_offset(15)
        e.set_snooker(w["every"], w["gamma_s"])
        e.run(1, 25, w["gamma"])
        chain, lobj = e.get_history(1, 25)
        Z = np.array(e.get_state()[2])
    finally:
        e.close()
    assert np.array_equal(chain, ref["chain"][:, :, 15:]) and np.array_equal(lobj, ref["log_obj"][:, 15:]) and np.array_equal(Z, ref["Z"])


def test_two_host_driven_shards_are_one_handle(demc, oracle):
    """35 + 35 chains with chain_id0 and caller-owned appends: a call ends at every K boundary and both handles are given all rows."""
    w, ref, run = cc.reference(oracle, "mvn5")
    es = [_engine(demc, w, N=35, chain_id0=35 * r, external=True) for r in range(2)]
    try:
        Kw, G = w["K"], w["G"]
        for a in range(1, G + 1, Kw):
            b = min(a + Kw - 1, G)
            for e in es:
                e.run(a, b, w["gamma"])
            if b % Kw == 0:
                rows = np.concatenate([np.array(e.get_state(with_Z=False)[0]) for e in es], axis=0)
                for e in es:
                    e.append_rows(rows)
        parts = [_collect(e, G) for e in es]
    finally:
        for e in es:
            e.close()
    got = dict(chain=np.concatenate([p["chain"] for p in parts], axis=0), log_obj=np.concatenate([p["log_obj"] for p in parts], axis=0),
               X=np.concatenate([p["X"] for p in parts], axis=0), logp=np.concatenate([p["logp"] for p in parts]), Z=parts[0]["Z"],
               M=parts[0]["M"], changed=parts[0]["changed"] + parts[1]["changed"])
    _same(got, ref, None, "two shards")
    assert np.array_equal(parts[0]["Z"], parts[1]["Z"])
    tried, accepted = run.counts()
    assert np.array_equal(parts[0]["crossover"].tried + parts[1]["crossover"].tried, tried)
    assert np.array_equal(parts[0]["crossover"].accepted + parts[1]["crossover"].accepted, accepted)


def test_demcz_sample_and_anneal_end_to_end(demc, oracle):
    w, ref, _ = cc.reference(oracle, "mvn5")
    mc, Z = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], w["G"], 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"],
                              crossover=(3, 3))
    assert np.array_equal(mc.chain, ref["chain"]) and np.array_equal(mc.log_obj, ref["log_obj"]) and np.array_equal(Z, ref["Z"])
    w, ref, _ = cc.reference(oracle, "mvn5_zero_weight")
    mc, Z = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], w["G"], 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"],
                              crossover=(3, 3, w["weights"]))
    assert np.array_equal(mc.chain, ref["chain"]) and np.array_equal(Z, ref["Z"])
    plain, _ = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], w["G"], 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"])
    assert not np.array_equal(plain.chain[:, :, 0], mc.chain[:, :, 0])
    an, _ = demc.demcz_anneal(w["target"], w["Z0"], w["N"], w["K"], w["G"], 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"],
                              crossover=(3, 3))
    assert an.chain.shape == (w["N"], 5, w["G"]) and np.isfinite(an.chain).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(demc, e, code, words, *args):
    with pytest.raises(demc.DemczError) as ei:
        e.set_crossover(*args)
    assert ei.value.code == code and all(wd in str(ei.value) for wd in words), str(ei.value)


def test_every_refusal_names_its_condition(demc):
    L = demc._lib
    w = cc.world("mvn5")
    e = _engine(demc, w, crossover=False)
    try:
        for ncr in (-1, 9):
            _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["ncr"], ncr, 3)
        for dm in (0, 4, -1):
            _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["delta_max"], 3, dm)
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["negative"], 3, 3, [1, -1, 1])
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["sum", "2^31"], 3, 3, [0, 0, 0])
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["sum", "2^31"], 2, 3, [2 ** 30, 2 ** 30])
        c = e.crossover
        assert (c.ncr, list(c.tried), list(c.accepted)) == (0, [], [])
        e.set_crossover(2, 3, [2 ** 30, 2 ** 30 - 1])            # W = 2^31 - 1
        e.set_crossover(3, 2)
        assert (e.crossover.ncr, e.crossover.delta_max, list(e.crossover.weights)) == (3, 2, [1, 1, 1])
        e.set_crossover(0)                                       # off again: the handle runs the full-block move
        e.run(1, 10, w["gamma"])
        assert e.kernel_name() == "demcz::window_kernel<MVNORMAL, 5, true>"
        # a handle that has run a generation
        _refused(demc, e, L.ERR_STATE, ["already run a generation"], 3, 3)
        _refused(demc, e, L.ERR_STATE, ["already run a generation"], 0, 1)
        # a derived history
        dh = e.rank_normalize(1, 10)
        rc = e._L.demcz_set_crossover(dh._h, 3, None, 3)
        assert rc == L.ERR_STATE and b"derived history" in e._L.demcz_last_error(dh._h)
        dh.close()
    finally:
        e.close()
    for lanes in (8, 100, 164):                       # fused lanes, the split, one wave per chain
        e = demc.HipEngine(N=64, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"], lanes_per_chain=lanes)
        try:
            _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["one-lane layout"], 3, 3)
        finally:
            e.close()
    e = demc.HipEngine(N=64, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(2), range(2, 5)], eps_scale=w["eps"], seed=1, target=w["target"], lanes_per_chain=1)
    try:
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["more than one block"], 3, 3)
    finally:
        e.close()
    w1 = demc.workloads.iso_quad_problem(1, 64)
    e = demc.HipEngine(N=64, d=1, K=10, Mcap=400, Gcap=0, blockindex=[range(1)], eps_scale=w1["eps_scale"], seed=1, target=w1["target"], lanes_per_chain=1)
    try:
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["d >= 2"], 3, 3)
    finally:
        e.close()
    e = demc.HipEngine(N=64, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=lambda x: 0.0, lanes_per_chain=1)
    try:
        _refused(demc, e, L.ERR_STATE, ["host-callback"], 3, 3)
    finally:
        e.close()
    # fewer than two archive rows never reach demcz_run (demcz_set_state refuses them; the check in demcz_run is a backstop behind it);
    # demcz_propose refuses a crossover handle
    e = demc.HipEngine(N=1, d=5, K=10, Mcap=40, Gcap=10, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"], lanes_per_chain=1)
    try:
        with pytest.raises(demc.DemczError) as ei:
            e.set_state(w["Z0"][:1], None, w["Z0"][:1])
        assert ei.value.code == L.ERR_INVALID_ARGUMENT
        e.set_state(w["Z0"][:1], None, w["Z0"][:2])
        e.set_crossover(3, 3)
        buf = np.zeros((1, 5), order="F")
        rc = e._L.demcz_propose(e._h, C.c_int64(1), C.c_int32(0), C.c_double(1.0), buf.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == L.ERR_STATE and b"crossover" in e._L.demcz_last_error(e._h)
        assert e.info()["window_launches"] == 0 and e.crossover.tried.sum() == 0
    finally:
        e.close()


def test_replica_groups_and_crossover_exclude_each_other(demc):
    L = demc._lib
    w = cc.world("mvn5")

    def pair():
        return [demc.HipEngine(N=35, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"],
                               chain_id0=35 * r, lanes_per_chain=1) for r in range(2)]
    es = pair()
    try:
        for r, e in enumerate(es):
            e.set_state(w["Z0"][-70:][35 * r:35 * r + 35], None, w["Z0"])
        demc.HipEngine.peer_group(es)
        _refused(demc, es[0], L.ERR_STATE, ["replica group"], 3, 3)
    finally:
        for e in es:
            e.close()
    es = pair()
    try:
        for r, e in enumerate(es):
            e.set_state(w["Z0"][-70:][35 * r:35 * r + 35], None, w["Z0"])
        es[1].set_crossover(3, 3)
        with pytest.raises(demc.DemczError) as ei:
            demc.HipEngine.peer_group(es)
        assert ei.value.code == L.ERR_STATE and "crossover" in str(ei.value)
    finally:
        for e in es:
            e.close()


def test_the_sampler_refuses_what_the_library_would(demc):
    w = demc.workloads.mvnormal_problem(5, 64)
    args = (w["Zinit"], 64, 10, 20)
    with pytest.raises(ValueError, match="one-lane"):
        demc.demcz_sample(w["target"], *args, 1, [range(5)], w["eps_scale"], w["gamma"], verbose=False, crossover=(3, 3), lanes_per_chain=8)
    with pytest.raises(ValueError, match="device target"):
        demc.demcz_sample(lambda x: 0.0, *args, 1, [range(5)], w["eps_scale"], w["gamma"], verbose=False, crossover=(3, 3))
    with pytest.raises(ValueError, match="one block"):
        demc.demcz_anneal(w["target"], *args, 2, [range(3), range(3, 5)], w["eps_scale"], w["gamma"], verbose=False, crossover=(3, 3))
