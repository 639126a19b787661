"""GPU: snooker generations (demcz_set_snooker, snooker_kernel) bit for bit against tests/snooker_reference.py.

The worlds are tests/snooker_cases.py's (held to their conditions by the reference alone in tests/test_snooker_cases.py): N = 70,
40 generations, every specialised dimension class and the run-time-d form, a program target, a program with bounded support, a
blocked handle, temperatures with zeros, anchors that are the chain's own row, +-inf in the archive.  chain, log_obj, the final X
and logp, Z, M and the per-generation changed counts are compared without tolerance; the snooker launches are counted; the
ballots answer changed_total.  Then the ways a run is cut (demcz_run calls, demcz_run_checked, a checkpoint, two host-driven
shards), every refusal of demcz_set_snooker, and demcz_sample end to end."""
import ctypes as C

import numpy as np
import pytest

import snooker_cases as sc
from helpers import same_bits
from program_texts import ROSENBROCK

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")


def _engine(demc, w, N=None, chain_id0=0, every=None, lanes=1, Gcap=None, external=False):
    N = w["N"] if N is None else N
    M0 = w["Z0"].shape[0]
    e = demc.HipEngine(N=N, d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (w["G"] // w["K"] + 1), Gcap=w["G"] if Gcap is None else Gcap,
                       blockindex=w["blocks"], eps_scale=w["eps"], seed=w["seed"], target=w["target"], chain_id0=chain_id0, lanes_per_chain=lanes)
    X0 = w["Z0"][M0 - w["N"]:]
    e.set_state(X0[chain_id0:chain_id0 + N], None, w["Z0"])
    if external:
        e.set_external_append(True)
    e.set_snooker(w["every"] if every is None else every, w["gamma_s"])
    return e


def _collect(e, G):
    chain, lobj = e.get_history(1, G)
    X, lp, Z, M = e.get_state()
    return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=e.get_changed(1, G))


def _run(demc, w, cuts=None):
    """The world on one handle, demcz_run called once or piece by piece (cuts: the last generation of every piece)."""
    e = _engine(demc, w)
    try:
        a = 1
        for b in (cuts or [w["G"]]):
            e.run(a, b, w["gamma"], None if w["temperature"] is None else w["temperature"][a - 1:b])
            a = b + 1
        got = _collect(e, w["G"])
        got["total"], got["from_ballots"] = e.changed_total(1, w["G"], with_source=True)
        got["snooker"], got["name"] = e.snooker, e.kernel_name()
        return got
    finally:
        e.close()


def _same(got, ref, what):
    same_bits(got, ref, keys=KEYS, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"


@pytest.mark.parametrize("name", list(sc.WORLDS))
def test_every_world_is_the_reference_bit_for_bit(demc, oracle, name):
    w, ref, run = sc.reference(oracle, name)
    got = _run(demc, w)
    _same(got, ref, name)
    assert got["snooker"] == (w["every"], w["gamma_s"][0], w["gamma_s"][1], len(run.snooker_generations)), name
    assert (got["total"], got["from_ballots"]) == (int(ref["changed"].sum()), True), f"{name}: changed_total from the ballots"
    if w["G"] % w["every"] == 0:            # the last launch was a snooker launch
        kind, d = w["kind"], w["d"]
        special = {"mvn": (2, 3, 4, 5, 8, 10, 20), "iso": (10,), "lr": (10, 26)}.get(kind)
        tg = {"mvn": "MVNORMAL", "iso": "ISO_QUAD", "lr": "LINREG_SSE"}.get(kind)
        want = f"demcz::snooker_kernel<4, {d}> (program)" if special is None else \
            f"demcz::snooker_kernel<{tg}, {d}>" if d in special else f"demcz::snooker_kernel_generic<{tg}>"
        assert got["name"] == want, name


@pytest.mark.parametrize("name,cuts", [("mvn5_all", [1, 2, 9, 10, 11, 29, 40]), ("mvn7", [2, 3, 4, 13, 30, 31, 40]),
                                       ("mvn5_tempered", [5, 6, 17, 18, 40])])
def test_a_run_cut_into_calls_anywhere_is_the_uncut_run(demc, oracle, name, cuts):
    w, ref, _ = sc.reference(oracle, name)
    _same(_run(demc, w, cuts), ref, f"{name} cut at {cuts}")


def test_run_checked_over_three_slabs_is_separate_calls(demc, oracle):
    """demcz_run_checked goes through the same executor: snooker generations every 4, three R-hat slabs of 12 generations."""
    w = dict(sc.world("mvn5"), every=4, G=36)
    ref = sc.mixed_run(oracle, w)
    ref.run(1, 36, w["gamma"])
    e = _engine(demc, w)
    try:
        g_stop, mx, _ = e.run_checked(1, 36, w["gamma"], 12, threshold=0.0)
        assert g_stop == 36 and len(mx) == 3
        got = _collect(e, 36)
        assert e.snooker[3] == 9
    finally:
        e.close()
    _same(got, ref.result(), "run_checked")
    sep = _run(demc, w, [12, 24, 36])
    _same(got, sep, "run_checked against three demcz_run calls")


def test_two_host_driven_shards_are_one_handle(demc, oracle):
    """35 + 35 chains with chain_id0 and caller-owned appends: a call ends at every K boundary and both handles are given all rows."""
    w, ref, _ = sc.reference(oracle, "mvn5")
    es = [_engine(demc, w, N=35, chain_id0=35 * r, external=True) for r in range(2)]
    try:
        K, G = w["K"], w["G"]
        for a in range(1, G + 1, K):
            b = min(a + K - 1, G)
            for e in es:
                e.run(a, b, w["gamma"])
            if b % K == 0:
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
    _same(got, ref, "two shards")
    assert np.array_equal(parts[0]["Z"], parts[1]["Z"])


def test_resume_through_a_checkpoint_is_the_uninterrupted_run(demc, oracle, tmp_path):
    """The first part's length is a multiple of K; snooker_every is passed again and the choice of move follows the streams."""
    w = sc.world("mvn7")                     # K = 10, every = 3: 20 % 3 != 0, so the resumed run's own g would choose other generations
    kw = dict(verbose=False, seed=w["seed"], snooker_every=w["every"], snooker_gamma=w["gamma_s"])
    args = (1, [range(w["d"])], w["eps"], w["gamma"])
    whole, Zw = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], 40, *args, **kw)
    first, Z1 = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], 20, *args, **kw)
    demc.save_checkpoint(tmp_path / "ck.npz", first, Z1, seed=w["seed"])
    prev, Zc, done, seed = demc.load_checkpoint(tmp_path / "ck.npz")
    assert done == 20
    kw["seed"] = seed
    second, Z2 = demc.demcz_sample(w["target"], Zc, w["N"], w["K"], 20, *args, prevrun=prev, **kw)
    assert np.array_equal(second.chain[:, :, 1:], whole.chain[:, :, 20:]) and np.array_equal(second.log_obj[:, 1:], whole.log_obj[:, 20:])
    assert np.array_equal(Z2, Zw) and np.array_equal(second.Xcurrent, whole.Xcurrent)
    _, ref, _ = sc.reference(oracle, "mvn7")
    assert np.array_equal(whole.chain, ref["chain"]) and np.array_equal(Zw, ref["Z"])


def test_demcz_sample_end_to_end(demc, oracle):
    d, N, K, G, seed = 5, 64, 10, 40, 77
    w = demc.workloads.mvnormal_problem(d, N)
    mc, Z = demc.demcz_sample(w["target"], w["Zinit"], N, K, G, 1, [range(d)], w["eps_scale"], w["gamma"], verbose=False, seed=seed,
                              snooker_every=10)
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=seed,
                       target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        e.set_snooker(10)
        e.run(1, G, w["gamma"])
        got = _collect(e, G)
        assert e.snooker == (10, 1.2, 2.2, 4)
    finally:
        e.close()
    assert np.array_equal(mc.chain, got["chain"]) and np.array_equal(mc.log_obj, got["log_obj"]) and np.array_equal(Z, got["Z"])
    assert np.array_equal(mc.Xcurrent, got["X"]) and np.array_equal(mc.log_objcurrent, got["logp"])
    plain, _ = demc.demcz_sample(w["target"], w["Zinit"], N, K, G, 1, [range(d)], w["eps_scale"], w["gamma"], verbose=False, seed=seed)
    assert np.array_equal(plain.chain[:, :, :9], mc.chain[:, :, :9]) and not np.array_equal(plain.chain[:, :, 9], mc.chain[:, :, 9])
    ref = sc.sr.MixedRun(oracle, N=N, d=d, K=K, G=G, blocks=None, eps=w["eps_scale"], seed=seed, Z0=w["Zinit"], target=w["target"], every=10)
    ref.run(1, G, w["gamma"])
    assert np.array_equal(mc.chain, ref.result()["chain"])


def test_switching_off_and_changing_between_runs(demc, oracle):
    w = sc.world("mvn5")
    ref = sc.mixed_run(oracle, w, every=2)
    ref.run(1, 10, w["gamma"])
    ref.every = 0
    ref.run(11, 20, w["gamma"])
    ref.every, ref.gamma_s = 5, (0.5, 0.5)
    ref.run(21, 40, w["gamma"])
    e = _engine(demc, w, every=2)
    try:
        e.run(1, 10, w["gamma"])
        e.set_snooker(0)
        e.run(11, 20, w["gamma"])
        e.set_snooker(5, (0.5, 0.5))
        e.run(21, 40, w["gamma"])
        got = _collect(e, 40)
        assert e.snooker == (5, 0.5, 0.5, 5 + 4)
    finally:
        e.close()
    _same(got, ref.result(), "every 2, off, every 5 with gamma_s = 0.5")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(demc, e, code, words, *args):
    with pytest.raises(demc.DemczError) as ei:
        e.set_snooker(*args)
    assert ei.value.code == code and all(wd in str(ei.value) for wd in words), str(ei.value)


def test_every_refusal_names_its_condition(demc):
    L = demc._lib
    w = sc.world("mvn5")
    e = _engine(demc, w, every=0)
    try:
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["every", ">= 0"], -1)
        for g in ((0.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (1.0, np.inf), (np.nan, 2.0)):
            _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["gamma_lo <= gamma_hi"], 3, g)
        assert e.snooker == (0, 1.2, 2.2, 0)
        # a derived history
        e.run(1, 10, w["gamma"])
        dh = e.rank_normalize(1, 10)
        rc = e._L.demcz_set_snooker(dh._h, 3, C.c_double(1.2), C.c_double(2.2))
        assert rc == L.ERR_STATE and b"derived history" in e._L.demcz_last_error(dh._h)
        dh.close()
    finally:
        e.close()
    for lanes in (8, 100, 164):                       # fused lanes, the split, one wave per chain
        e = demc.HipEngine(N=64, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"], lanes_per_chain=lanes)
        try:
            _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["one-lane layout"], 3)
        finally:
            e.close()
    w1 = demc.workloads.iso_quad_problem(1, 64)
    e = demc.HipEngine(N=64, d=1, K=10, Mcap=400, Gcap=0, blockindex=[range(1)], eps_scale=w1["eps_scale"], seed=1, target=w1["target"], lanes_per_chain=1)
    try:
        _refused(demc, e, L.ERR_INVALID_ARGUMENT, ["d >= 2"], 3)
    finally:
        e.close()
    e = demc.HipEngine(N=64, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=lambda x: 0.0, lanes_per_chain=1)
    try:
        _refused(demc, e, L.ERR_STATE, ["host-callback"], 3)
    finally:
        e.close()
    # fewer than three archive rows: refused by demcz_run before anything is enqueued
    e = demc.HipEngine(N=2, d=5, K=10, Mcap=40, Gcap=10, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(w["Z0"][:2], None, w["Z0"][:2])
        e.set_snooker(3)
        with pytest.raises(demc.DemczError) as ei:
            e.run(1, 10, w["gamma"])
        assert ei.value.code == L.ERR_STATE and "fewer than three" in str(ei.value)
        assert e.info()["window_launches"] == 0 and e.snooker[3] == 0
        e.set_snooker(0)
        e.run(1, 10, w["gamma"])
    finally:
        e.close()


def test_replica_groups_and_snooker_exclude_each_other(demc):
    L = demc._lib
    w = sc.world("mvn5")

    def pair():
        return [demc.HipEngine(N=35, d=5, K=10, Mcap=400, Gcap=0, blockindex=[range(5)], eps_scale=w["eps"], seed=1, target=w["target"],
                               chain_id0=35 * r, lanes_per_chain=1) for r in range(2)]
    es = pair()
    try:
        for r, e in enumerate(es):
            e.set_state(w["Z0"][-70:][35 * r:35 * r + 35], None, w["Z0"])
        demc.HipEngine.peer_group(es)
        _refused(demc, es[0], L.ERR_STATE, ["replica group"], 3)
    finally:
        for e in es:
            e.close()
    es = pair()
    try:
        for r, e in enumerate(es):
            e.set_state(w["Z0"][-70:][35 * r:35 * r + 35], None, w["Z0"])
        es[1].set_snooker(3)
        with pytest.raises(demc.DemczError) as ei:
            demc.HipEngine.peer_group(es)
        assert ei.value.code == L.ERR_STATE and "snooker" in str(ei.value)
    finally:
        for e in es:
            e.close()


def test_the_sampler_refuses_what_the_library_would(demc):
    w = demc.workloads.mvnormal_problem(5, 64)
    args = (w["Zinit"], 64, 10, 20, 1, [range(5)], w["eps_scale"], w["gamma"])
    with pytest.raises(ValueError, match="one-lane"):
        demc.demcz_sample(w["target"], *args, verbose=False, snooker_every=5, lanes_per_chain=8)
    with pytest.raises(ValueError, match="device target"):
        demc.demcz_sample(lambda x: 0.0, *args, verbose=False, snooker_every=5)
    with pytest.raises(ValueError, match="one-lane"):
        demc.demcz_anneal(w["target"], *args, verbose=False, snooker_every=5, lanes_per_chain=100)


def test_check_compiles_the_snooker_kernel_of_a_program(demc):
    """check() builds the unit the handle will load: window_full, window_blocks and the snooker kernel.  A program that defines a
    name the snooker kernel's own text uses compiles for no kernel of the unit and fails at check(), not in a run."""
    demc.ProgramTarget(ROSENBROCK, 7).check()
    bad = demc.ProgramTarget("#define snooker_accept 0\n" + ROSENBROCK, 7)
    with pytest.raises(demc.DemczError) as ei:
        bad.check()
    assert "demcz_kernels_snooker.h" in str(ei.value)
