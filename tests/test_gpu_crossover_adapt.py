"""GPU: adaptation of the crossover class weights on the device (demcz_set_crossover_adapt, window_kernel_cr<T, D, adapt>,
cr_adapt_kernel) bit for bit against tests/crossover_adapt_reference.py.

The worlds are tests/crossover_adapt_cases.py's WORLDS (held to their conditions by the reference alone in
tests/test_crossover_adapt_cases.py): N = 100 / 70 / 130, a hundred generations and more, four or five updates; a specialised
dimension and the run-time-d form, a start that clamps, a constant column, the floor, temperatures, snooker generations on update
positions.  chain, log_obj, the final X and logp, Z, M and the per-generation changed counts are compared without tolerance; weights,
dist, tried and updates for equality, rsd for equal bits.  Every world runs as one call, cut into uneven calls (the state compared
after every call) and through demcz_run_checked; then a resume through get / set state on a fresh handle, a change of weights in
mid-life, every refusal, and the worlds of tests/crossover_cases.py with adaptation off."""
import numpy as np
import pytest

import crossover_adapt_cases as ac
import crossover_cases as cc
from helpers import same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")


def _engine(demc, w, adapt=True, G=None, Z0=None, X0=None, lp0=None):
    Z0 = w["Z0"] if Z0 is None else Z0
    M0 = Z0.shape[0]
    G = w["G"] if G is None else G
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (G // w["K"] + 1), Gcap=G, blockindex=[range(w["d"])],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], lanes_per_chain=1)
    e.set_state(Z0[M0 - w["N"]:] if X0 is None else X0, lp0, Z0)
    e.set_crossover(w["ncr"], w["delta_max"], w["weights"])
    if adapt:
        e.set_crossover_adapt(w["adapt_every"], w["adapt_until"], w["min_weight"])
    if w["every"]:
        e.set_snooker(w["every"], w["gamma_s"])
    return e


def _collect(e, G):
    chain, lobj = e.get_history(1, G)
    X, lp, Z, M = e.get_state()
    return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=e.get_changed(1, G),
                crossover=e.crossover, adapt=e.crossover_adapt)


def _temps(w, a, b):
    return None if w["temperature"] is None else w["temperature"][a - 1:b]


def _same_state(a, st, what):
    """a: CrossoverAdapt of the handle; st: AdaptRun.state()"""
    assert list(a.weights) == st["weights"], f"{what}: weights {list(a.weights)} / {st['weights']}"
    assert list(a.dist) == st["dist"], f"{what}: dist {list(a.dist)} / {st['dist']}"
    assert list(a.tried) == st["tried"], f"{what}: tried {list(a.tried)} / {st['tried']}"
    assert a.updates == st["updates"], f"{what}: updates {a.updates} / {st['updates']}"
    same_bits(dict(rsd=a.rsd), dict(rsd=np.array(st["rsd"])), keys=("rsd",), what=what)


def _same(got, ref, run, what):
    same_bits(got, ref, keys=KEYS, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation"
    _same_state(got["adapt"], run.state(), what)
    tried, accepted = run.counts()
    c = got["crossover"]
    assert np.array_equal(c.tried, tried) and np.array_equal(c.accepted, accepted), f"{what}: the life-time counters"
    assert list(c.weights) == run.weights, f"{what}: demcz_get_crossover reports the device's weights"


@pytest.mark.parametrize("name", list(ac.WORLDS))
def test_every_world_is_the_reference_bit_for_bit(demc, oracle, name):
    w, ref, run = ac.reference(oracle, name)
    e = _engine(demc, w)
    try:
        e.run(1, w["G"], w["gamma"], _temps(w, 1, w["G"]))
        got = _collect(e, w["G"])
        name_behind = e.kernel_name()
    finally:
        e.close()
    _same(got, ref, run, name)
    a = got["adapt"]
    assert (a.every, a.until, a.min_weight) == (w["adapt_every"], w["adapt_until"], w["min_weight"])
    assert np.array_equal(a.shares, np.array(run.weights) / sum(run.weights))
    assert np.array_equal(a.jump_per_try, np.array(run.dist) / 65536.0 / np.array(run.tried))
    if not (w["every"] and w["G"] % w["every"] == 0):
        assert name_behind == ac.planned_kernel(w), name


@pytest.mark.parametrize("name", list(ac.WORLDS))
def test_a_run_cut_into_uneven_calls_is_the_uncut_run_after_every_call(demc, oracle, name):
    """cuts on, before and behind update positions and K boundaries; the state on the device after every call is the state of a
    reference run driven by the same calls"""
    w, ref, run = ac.reference(oracle, name)
    piecewise = ac.adapt_run(oracle, w)
    e = _engine(demc, w)
    try:
        a = 1
        for b in ac.uneven_cuts(w):
            e.run(a, b, w["gamma"], _temps(w, a, b))
            piecewise.run(a, b, w["gamma"], _temps(w, a, b))
            X, lp, _, _ = e.get_state()
            same_bits(dict(X=np.array(X), logp=np.array(lp)), dict(X=piecewise.X, logp=np.array(piecewise.lp)), keys=("X", "logp"), what=f"{name} after {b}")
            _same_state(e.crossover_adapt, piecewise.state(), f"{name} after the call that ends at {b}")
            a = b + 1
        got = _collect(e, w["G"])
    finally:
        e.close()
    _same(got, ref, run, f"{name} cut at {ac.uneven_cuts(w)}")


@pytest.mark.parametrize("name", list(ac.WORLDS))
def test_run_checked_is_the_run(demc, oracle, name):
    w, ref, run = ac.reference(oracle, name)
    slab = 20 if w["G"] % 20 == 0 else 10
    e = _engine(demc, w)
    try:
        g_stop, mx, _ = e.run_checked(1, w["G"], w["gamma"], slab, threshold=0.0, temperature=_temps(w, 1, w["G"]))
        assert g_stop == w["G"] and len(mx) == w["G"] // slab
        got = _collect(e, w["G"])
    finally:
        e.close()
    _same(got, ref, run, f"{name} through run_checked")


@pytest.mark.parametrize("name,cut", [("mvn5", 35), ("mvn5_far", 50), ("mvn5_snooker", 30)])
def test_resume_through_get_and_set_state_on_a_fresh_handle(demc, oracle, name, cut):
    """A checkpoint between two updates, one on an update position, one with snooker generations: the state of the adaptation goes
    through demcz_get_crossover_adapt / demcz_set_crossover_adapt_state, the positions through demcz_set_rng_offset."""
    w, ref, run = ac.reference(oracle, name)
    assert cut % w["K"] == 0
    e = _engine(demc, w)
    try:
        e.run(1, cut, w["gamma"], _temps(w, 1, cut))
        st = e.crossover_adapt
        X, lp, Z, M = e.get_state()
        X, lp, Z = np.array(X), np.array(lp), np.array(Z[:M])
    finally:
        e.close()
    rest = w["G"] - cut
    e = _engine(demc, w, G=rest, Z0=Z, X0=X, lp0=lp)
    try:
        e.set_rng_offset(cut)
        e.set_crossover_adapt_state(st.weights, st.dist, st.tried, st.rsd, st.updates)
        _same_state(e.crossover_adapt, dict(weights=list(st.weights), dist=list(st.dist), tried=list(st.tried), rsd=list(st.rsd), updates=st.updates),
                    f"{name}: the state read back")
        e.run(1, rest, w["gamma"], _temps(w, cut + 1, w["G"]))
        chain, lobj = e.get_history(1, rest)
        X2, lp2, Z2, M2 = e.get_state()
        got = e.crossover_adapt
    finally:
        e.close()
    what = f"{name} resumed at {cut}"
    same_bits(dict(chain=chain, log_obj=lobj, X=np.array(X2), logp=np.array(lp2), Z=np.array(Z2[:M2])),
              dict(chain=ref["chain"][:, :, cut:], log_obj=ref["log_obj"][:, cut:], X=ref["X"], logp=ref["logp"], Z=ref["Z"]), keys=KEYS, what=what)
    _same_state(got, run.state(), what)


def test_a_resume_without_the_state_is_another_run(demc, oracle):
    """what the state carries: without it the resumed handle starts its sums (and its spread) afresh"""
    w, ref, run = ac.reference(oracle, "mvn5")
    first = ac.adapt_run(oracle, w)
    first.run(1, 35, w["gamma"])
    r1 = first.result()
    e = _engine(demc, w, G=w["G"] - 35, Z0=r1["Z"], X0=r1["X"], lp0=r1["logp"])
    try:
        e.set_rng_offset(35)
        e.run(1, w["G"] - 35, w["gamma"])
        a = e.crossover_adapt
    finally:
        e.close()
    assert a.updates == run.updates - 1 and list(a.tried) != run.tried


def test_new_weights_in_mid_life_match_the_reference_with_the_same_change(demc, oracle):
    """behind `until` (and on a handle without adaptation at any time) demcz_set_crossover_weights holds from the next launch on"""
    w = ac.world("mvn5")
    for adapt in (True, False):
        ref = ac.adapt_run(oracle, w) if adapt else cc.crossover_run(oracle, w)
        at = w["adapt_until"] + 3 if adapt else 33
        ref.run(1, at, w["gamma"])
        if adapt:
            ref.set_weights([5, 0, 1])
        else:
            ref.weights, ref.cum = [5, 0, 1], [5, 5, 6]
        ref.run(at + 1, w["G"], w["gamma"])
        e = _engine(demc, w, adapt=adapt)
        try:
            e.run(1, at, w["gamma"])
            e.set_crossover_weights([5, 0, 1])
            assert list(e.crossover.weights) == [5, 0, 1]
            e.run(at + 1, w["G"], w["gamma"])
            got = _collect(e, w["G"])
        finally:
            e.close()
        same_bits(got, ref.result(), keys=KEYS, what=f"adapt={adapt}")
        tried, accepted = ref.counts()
        assert np.array_equal(got["crossover"].tried, tried) and np.array_equal(got["crossover"].accepted, accepted)
        assert all(f["m"] != 1 for g, _, f in ref.steps if g > at) and any(f["m"] == 1 for g, _, f in ref.steps if g <= at)
        if adapt:
            _same_state(got["adapt"], ref.state(), "weights set by hand behind until")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(demc, call, code, words):
    with pytest.raises(demc.DemczError) as ei:
        call()
    assert ei.value.code == code and all(wd in str(ei.value) for wd in words), str(ei.value)


def test_every_refusal_names_its_condition(demc):
    L = demc._lib
    w = ac.world("mvn5")
    M0 = w["Z0"].shape[0]

    def fresh(crossover=True):
        e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * 20, Gcap=0, blockindex=[range(w["d"])], eps_scale=w["eps"], seed=1,
                           target=w["target"], lanes_per_chain=1)
        e.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
        if crossover:
            e.set_crossover(3, 3)
        return e

    e = fresh(crossover=False)
    try:
        _refused(demc, lambda: e.set_crossover_adapt(10, 100), L.ERR_STATE, ["no crossover"])
        _refused(demc, lambda: e._chk(e._L.demcz_set_crossover_weights(e._h, None)), L.ERR_STATE, ["no crossover"])
        a = e.crossover_adapt
        assert (a.every, a.until, a.updates, len(a.weights)) == (0, 0, 0, 0)
    finally:
        e.close()
    e = fresh()
    try:
        for every, until, mw, words in ((-1, 10, 656, ["every"]), (10, 5, 656, ["until"]), (10, 25, 656, ["until"]), (10, 100, 0, ["min_weight"]),
                                        (10, 100, 8193, ["min_weight"]), (1, (2 ** 31 - 1) // w["N"] + 1, 656, ["2^31"]), (2 ** 31, 2 ** 31, 656, ["2^31"])):
            _refused(demc, lambda: e.set_crossover_adapt(every, until, mw), L.ERR_INVALID_ARGUMENT, words)
        e.set_crossover_adapt(1, (2 ** 31 - 1) // w["N"])                   # N * until at the bound
        e.set_crossover_adapt(10, 100, 8192)
        e.set_crossover_adapt(10, 100, 1)
        e.set_crossover_adapt(0, 0)                                         # off again
        assert e.crossover_adapt.every == 0
        _refused(demc, lambda: e.set_crossover_adapt_state([1, 1, 1], [0, 0, 0], [0, 0, 0], np.ones(w["d"]), 0), L.ERR_STATE, ["no adaptation"])
        e.set_crossover_adapt(10, 20)
        _refused(demc, lambda: e.set_crossover_adapt_state([0, 0, 0], [0, 0, 0], [0, 0, 0], np.ones(w["d"]), 0), L.ERR_INVALID_ARGUMENT, ["sum"])
        _refused(demc, lambda: e.set_crossover_adapt_state([1, 1, 1], [0, -1, 0], [0, 0, 0], np.ones(w["d"]), 0), L.ERR_INVALID_ARGUMENT, ["negative"])
        _refused(demc, lambda: e.set_external_append(True), L.ERR_STATE, ["adapts"])
        e.set_crossover(4, 2)                                               # a changed ncr clears it
        assert e.crossover_adapt.every == 0
        e.set_crossover(3, 3)
        e.set_crossover_adapt(10, 20)
        e.set_crossover(3, 2, [1, 2, 3])                                    # the same ncr keeps it, with the new weights
        a = e.crossover_adapt
        assert (a.every, a.until, list(a.weights)) == (10, 20, [1, 2, 3])
        e.set_crossover(3, 3)
        e.run(1, 5, w["gamma"])
        assert e.kernel_name() == "demcz::window_kernel_cr<MVNORMAL, 5, adapt>"
        # a handle that has run a generation; weights by hand while the adaptation is still running
        _refused(demc, lambda: e.set_crossover_adapt(10, 100), L.ERR_STATE, ["already run a generation"])
        _refused(demc, lambda: e.set_crossover_adapt(0, 0), L.ERR_STATE, ["already run a generation"])
        _refused(demc, lambda: e.set_crossover_adapt_state([1, 1, 1], [0, 0, 0], [0, 0, 0], np.ones(w["d"]), 0), L.ERR_STATE, ["already run a generation"])
        _refused(demc, lambda: e.set_crossover_weights([1, 2, 3]), L.ERR_STATE, ["still running"])
        e.run(6, 19, w["gamma"])
        _refused(demc, lambda: e.set_crossover_weights([1, 2, 3]), L.ERR_STATE, ["still running"])
        e.run(20, 20, w["gamma"])
        assert e.crossover_adapt.updates == 2
        _refused(demc, lambda: e.set_crossover_weights([1, -2, 3]), L.ERR_INVALID_ARGUMENT, ["negative"])
        _refused(demc, lambda: e.set_crossover_weights([0, 0, 0]), L.ERR_INVALID_ARGUMENT, ["sum"])
        e.set_crossover_weights([1, 2, 3])
        assert list(e.crossover_adapt.weights) == [1, 2, 3] and list(e.crossover.weights) == [1, 2, 3]
        # a derived history
        dh_engine = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * 20, Gcap=10, blockindex=[range(w["d"])], eps_scale=w["eps"], seed=1,
                                   target=w["target"], lanes_per_chain=1)
        try:
            dh_engine.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
            dh_engine.run(1, 10, w["gamma"])
            dh = dh_engine.rank_normalize(1, 10)
            assert e._L.demcz_set_crossover_adapt(dh._h, 10, 100, 656) == L.ERR_STATE and b"derived history" in e._L.demcz_last_error(dh._h)
            dh.close()
        finally:
            dh_engine.close()
    finally:
        e.close()
    e = fresh()
    try:
        e.set_external_append(True)
        _refused(demc, lambda: e.set_crossover_adapt(10, 100), L.ERR_STATE, ["appends externally"])
        e.set_crossover_weights([3, 2, 1])                                  # the by-hand route such drivers keep
        assert list(e.crossover.weights) == [3, 2, 1]
    finally:
        e.close()


def test_the_sampler_takes_and_refuses_crossover_adapt(demc, oracle):
    w, ref, run = ac.reference(oracle, "mvn5")
    mc, Z = demc.demcz_sample(w["target"], w["Z0"], w["N"], w["K"], w["G"], 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"],
                              crossover=(3, 3), crossover_adapt=(w["adapt_every"], w["adapt_until"]))
    assert np.array_equal(mc.chain, ref["chain"]) and np.array_equal(mc.log_obj, ref["log_obj"]) and np.array_equal(Z, ref["Z"])
    an, _ = demc.demcz_anneal(w["target"], w["Z0"], w["N"], w["K"], 40, 1, [range(5)], w["eps"], w["gamma"], verbose=False, seed=w["seed"],
                              crossover=(3, 3), crossover_adapt=(10, 20, 1000))
    assert an.chain.shape == (w["N"], 5, 40) and np.isfinite(an.chain).all()
    args = (w["target"], w["Z0"], w["N"], w["K"], 20, 1, [range(5)], w["eps"], w["gamma"])
    with pytest.raises(ValueError, match="crossover="):
        demc.demcz_sample(*args, verbose=False, crossover_adapt=(10, 20))
    with pytest.raises(ValueError, match="crossover="):
        demc.demcz_anneal(*args, verbose=False, crossover_adapt=(10, 20))
    with pytest.raises(ValueError, match="multiple"):
        demc.demcz_sample(*args, verbose=False, crossover=(3, 3), crossover_adapt=(10, 25))
    with pytest.raises(ValueError, match="min_weight"):
        demc.demcz_sample(*args, verbose=False, crossover=(3, 3), crossover_adapt=(10, 20, 9000))


# ---- adaptation off: today's bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.WORLDS))
def test_with_adaptation_off_the_crossover_worlds_are_what_they_were(demc, oracle, name):
    """the worlds of tests/crossover_cases.py through this build, adaptation never set: the reference of the crossover generations
    (which knows nothing of adaptation), the two-argument kernels by name"""
    w, ref, run = cc.reference(oracle, name)
    M0 = w["Z0"].shape[0]
    e = demc.HipEngine(N=w["N"], d=w["d"], K=w["K"], Mcap=M0 + w["N"] * (w["G"] // w["K"] + 1), Gcap=w["G"], blockindex=[range(w["d"])],
                       eps_scale=w["eps"], seed=w["seed"], target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(w["Z0"][M0 - w["N"]:], None, w["Z0"])
        e.set_crossover(w["ncr"], w["delta_max"], w["weights"])
        if w["every"]:
            e.set_snooker(w["every"], w["gamma_s"])
        e.run(1, w["G"], w["gamma"], _temps(w, 1, w["G"]))
        got = _collect(e, w["G"])
        name_behind = e.kernel_name()
    finally:
        e.close()
    same_bits(got, ref, keys=KEYS, what=name)
    assert got["M"] == ref["M"] and np.array_equal(got["changed"], ref["changed"])
    tried, accepted = run.counts()
    assert np.array_equal(got["crossover"].tried, tried) and np.array_equal(got["crossover"].accepted, accepted)
    assert got["adapt"].every == 0 and got["adapt"].updates == 0 and list(got["adapt"].weights) == run.weights
    assert "adapt" not in name_behind
    if not (w["every"] and w["G"] % w["every"] == 0):
        assert name_behind == cc.planned_kernel(w)
