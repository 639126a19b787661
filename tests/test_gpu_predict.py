"""GPU: posterior predictive programs (demcz_predict, demcz_ppc; demcz_kernels_predict.h) against the NumPy restatements of
tests/predict_cases.py over the streams of tests/predict_reference.py.  Every comparison is exact: values bit for bit, counts as
integers.  Shapes are the smallest at which the kernels can go wrong: one draw, a wave across a generation boundary, both limits, a
ragged workgroup, a second ragged pass of the stride loop, and for the ballots of ppc_kernel a wave that is short by a lane, long
by a lane, and a workgroup that is."""
import numpy as np
import pytest

import predict_cases as pc
import predict_reference as pr
from derive_cases import history as _history
from helpers import bits_differ

pytestmark = pytest.mark.gpu

SEED = 20240611
PROBS = [0.05, 0.5, 0.95]


def _engine(demc, w, N, d, K, G, seed, Gcap=None, chain_id0=0):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G if Gcap is None else Gcap, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=seed, target=w["target"], chain_id0=chain_id0)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


def _predict_array(demc, prog, chain, log_obj, seed=SEED, chain_id0=0):
    with demc.predict_chain(chain, log_obj, prog, seed, chain_id0=chain_id0) as h:
        return h.get()


def _same(got, ref):
    why = bits_differ(got, ref)
    assert why is None, why


def _counts(r):
    return r.gt.tolist(), r.eq.tolist(), r.nan.tolist()


def _ref_counts(values, observed=None):
    return tuple(v.tolist() for v in pr.ppc_counts(values, observed))


# ---- predict, array form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,G,m", [(1, 1, 1, 1), (70, 3, 5, 2), (64, 32, 3, 32), (257, 5, 9, 3)])
def test_array_form_is_the_restatement_bit_for_bit(demc, N, d, G, m):
    prog, f = pc.generic_program(demc, d, m)
    chain, log_obj = _history(N, d, G, seed=100 + N)
    got = _predict_array(demc, prog, chain, log_obj)
    assert got.shape == (N, m, G) and got.flags.f_contiguous
    _same(got, pc.reference(f, chain, log_obj, SEED))


@pytest.fixture(scope="module")
def stride_twice(demc):
    """The shape whose window is strided over twice with a ragged last pass, its history and the restatement (one uniform a draw)."""
    threads, max_wg = demc._lib.derive_launch_constants()
    cap = threads * max_wg
    N, d = 1031, 2
    G = cap // N + 2
    total = N * G
    assert cap < total < 2 * cap and (total - cap) % cap != 0 and (total - cap) % threads != 0 and (total - cap) % 64 != 0
    prog, f = pc.program(demc, "one_uniform")
    chain, log_obj = _history(N, d, G, seed=5)
    ref = pc.reference(f, chain, log_obj, SEED)
    ref.setflags(write=False)
    return prog, chain, log_obj, ref


def test_stride_loop_runs_twice_with_a_ragged_last_pass(demc, stride_twice):
    prog, chain, log_obj, ref = stride_twice
    _same(_predict_array(demc, prog, chain, log_obj), ref)


def test_per_lane_state_under_divergence(demc):
    prog, f = pc.program(demc, "divergent")
    chain, log_obj = _history(70, 1, 5, seed=6)
    got = _predict_array(demc, prog, chain, log_obj)
    _same(got, pc.reference(f, chain, log_obj, SEED))
    assert len(set(got[:64, 0, 0].tolist())) >= 2                     # (lanes of one wave left the loop at different times)


def test_another_seed_and_another_first_chain_are_other_streams(demc):
    prog, f = pc.generic_program(demc, 3, 2)
    chain, log_obj = _history(70, 3, 5, seed=7)
    a = _predict_array(demc, prog, chain, log_obj)
    b = _predict_array(demc, prog, chain, log_obj, seed=SEED + 1)
    c = _predict_array(demc, prog, chain, log_obj, chain_id0=2**32 - 70)     # (the last chains a stream can be keyed by)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    _same(b, pc.reference(f, chain, log_obj, SEED + 1))
    _same(c, pc.reference(f, chain, log_obj, SEED, chain_id0=2**32 - 70))
    _same(_predict_array(demc, prog, chain, log_obj), a)              # (a call repeated is the same bits)


# ---- predict, engine form -----------------------------------------------------------------------------------------------------
def test_engine_form_reads_the_right_slots_and_log_obj(demc):
    N, d, K, G = 64, 3, 5, 40
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = pc.generic_program(demc, d, 4)                          # (column 3 subtracts logp)
    e = _engine(demc, w, N, d, K, G, seed=21)
    e.run(1, G, w["gamma"])
    h = e.predict(prog, 11, 40)                                       # (seed: the engine's own)
    assert (h.N, h.m, h.g_from, h.g_to, h.chain_id0) == (N, 4, 11, 40, 0)
    ref = pc.reference(f, *e.get_history(11, 40), 21, g_from=11)
    _same(h.get(), ref)
    with e.predict(prog, 11, 40, seed=21) as h2:
        _same(h2.get(), ref)
    with e.predict(prog, 11, 40, seed=22) as h3:
        assert not np.array_equal(h3.get(), ref)
    e.close()
    _same(h.get(), ref)                                               # the derived history survives its source
    h.close()


def test_window_independence(demc):
    N, d, K, G = 64, 3, 5, 9
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = pc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, K, G, seed=31)
    e.run(1, G, w["gamma"])
    with e.predict(prog, 1, 9) as whole, e.predict(prog, 3, 7) as part:
        v = whole.get()
        _same(part.get(), v[:, :, 2:7])
        _same(whole.get(3, 7), v[:, :, 2:7])
    _same(v, pc.reference(f, *e.get_history(1, 9), 31))
    e.close()


def test_after_the_history_origin_moved(demc):
    N, d, K = 64, 3, 5
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = pc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, K, 60, seed=32, Gcap=30)
    e.run(1, 30, w["gamma"])
    e.synchronize()
    e.set_history_origin(30)
    e.run(31, 60, w["gamma"])
    with e.predict(prog, 36, 57) as h:
        v = h.get()
        _same(v, pc.reference(f, *e.get_history(36, 57), 32, g_from=36))      # (generation 36 is slot 5 now: its stream is 36's)
    with e.predict(prog, 40, 50) as h:
        _same(h.get(), v[:, :, 4:15])
    with pytest.raises(demc.DemczError) as ei:
        e.predict(prog, 25, 40)                                       # (generations 25..30 left the window)
    assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT
    e.close()


def test_after_live_launches(demc):
    """N = 256, d = 5, K = 2: the shape at which tests/test_gpu_live.py sees LIVE launches inside demcz_run_checked.  The last
    demcz_run is not synchronised: demcz_predict verifies it (live_verify) before it reads the history."""
    N, d, K, G, every = 256, 5, 2, 400, 100
    w = demc.workloads.mvnormal_problem(d, N)
    prog = demc.PredictiveProgram(pc.ONE_UNIFORM, d, 1)
    e = _engine(demc, w, N, d, K, G, seed=43)
    e.run_checked(1, 300, w["gamma"], every, 0.0)
    e.run(301, G, w["gamma"])
    h = e.predict(prog, 101, G)
    assert e.live_status()[0], "this shape is expected to run LIVE launches"
    v = h.get()
    _same(v, pc.reference(pc.one_uniform_numpy, *e.get_history(101, G), 43, g_from=101))
    with e.predict(prog, 201, 300) as part:
        _same(part.get(), v[:, :, 100:200])
    h.close()
    e.close()


def test_predict_of_a_derived_history(demc):
    first, f1 = pc.generic_program(demc, 4, 3)
    second, f2 = pc.generic_program(demc, 3, 4)
    chain, log_obj = _history(70, 4, 6, seed=16)
    with demc.predict_chain(chain, log_obj, first, SEED) as h1:
        with pytest.raises(ValueError):
            h1.predict(second, 2, 5)                                  # (a derived history knows no run's seed)
        with pytest.raises(ValueError):
            h1.ppc(second, 2, 5)
        h2 = h1.predict(second, 2, 5, seed=9)
    got = h2.get()
    assert (h2.g_from, h2.g_to) == (2, 5)
    h2.close()
    v1 = pc.reference(f1, chain, log_obj, SEED)
    _same(got, pc.reference(f2, np.asfortranarray(v1[:, :, 1:5]), None, 9, g_from=2))
    assert np.isnan(got[:, 3, :]).all() and not np.isnan(got[:, :3, :]).any()       # logp of a derived history is NaN


# ---- shards -------------------------------------------------------------------------------------------------------------------
def test_host_sharding_equals_one_handle(demc):
    d, N, G = 3, 64, 40
    w = demc.workloads.mvnormal_problem(d, N)
    opts = demc.demcopt(d, N=N, K=5, Ngeneration=G, eps_scale=w["eps_scale"], verbose=False, autostop="Rhat", autostop_every=20,
                        autostop_Rhat=0.0)
    prog, f = pc.generic_program(demc, d, 3)
    count, _ = pc.program(demc, "count8")
    count = demc.PredictiveProgram(count.source, d, 2)
    a, Za, ra = demc.demcz_sample(w["target"], w["Zinit"], opts, seed=8, return_runner=True)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=2)
    b, Zb, rb = demc.demcz_sample(w["target"], w["Zinit"], opts, seed=8, sharding=sh, return_runner=True)
    assert [e.chain_id0 for e in rb.engines] == [0, 32] and len(ra.engines) == 1
    one = ra.engines[0]
    with one.predict(prog, 5, G) as h:
        whole = h.get()
    parts = []
    for e in rb.engines:
        with e.predict(prog, 5, G) as h:
            assert h.chain_id0 == e.chain_id0
            parts.append(h.get())
    _same(np.concatenate(parts, axis=0), whole)
    _same(whole, pc.reference(f, a.chain[:, :, 4:], a.log_obj[:, 4:], 8, g_from=5))
    obs = [4.0, 4.0]
    r1 = one.ppc(count, 5, G, observed=obs)
    r2 = rb.engines[0].ppc(count, 5, G, observed=obs) + rb.engines[1].ppc(count, 5, G, observed=obs)
    assert _counts(r1) == _counts(r2) and r1.total == r2.total == N * (G - 4)
    assert r1.eq[0] > 0 and r1.eq[1] == 0                             # (ties where the statistic is a count, none where it is a sum)
    ra.close(); rb.close()


# ---- ppc ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,G", [(1, 1), (63, 1), (65, 1), (257, 9)])
def test_ppc_counts_are_those_of_predict_and_of_the_restatement(demc, N, G):
    for name, observed in (("count8", [4.0, 4.0]), ("count8", None), ("count8", [np.nan, 3.5]),
                           ("specials", [np.inf, 0.0, 0.0, 0.0]), ("specials", [-np.inf, np.nan, np.nan, 0.25]), ("specials", None)):
        prog, f = pc.program(demc, name)
        chain, log_obj = _history(N, prog.d, G, seed=50 + N)
        r = demc.ppc_chain(chain, log_obj, prog, SEED, observed=observed)
        values = _predict_array(demc, prog, chain, log_obj)
        ref = pc.reference(f, chain, log_obj, SEED)
        _same(values, ref)
        assert _counts(r) == _ref_counts(values, observed) == _ref_counts(ref, observed), (name, observed)
        assert r.total == N * G and ((r.gt + r.eq + r.nan) <= r.total).all()
        if name == "specials":
            assert r.nan[1] == r.total and r.gt[1] == r.eq[1] == 0    # (the column the program never writes)
        if observed is not None and np.isnan(observed[0]):
            assert r.gt[0] == r.eq[0] == 0


def test_ppc_special_values_are_all_met(demc):
    """The shape above with the most draws holds every branch of the SPECIALS program: ties at +inf and -inf, NaN outputs, -0.0."""
    prog, f = pc.program(demc, "specials")
    chain, log_obj = _history(257, 1, 9, seed=50 + 257)
    ref = pc.reference(f, chain, log_obj, SEED)
    assert np.isposinf(ref[:, 0, :]).any() and np.isneginf(ref[:, 0, :]).any() and np.isfinite(ref[:, 0, :]).any()
    assert np.isnan(ref[:, 2, :]).any() and (np.signbit(ref[:, 2, :]) & (ref[:, 2, :] == 0)).any()
    r = demc.ppc_chain(chain, log_obj, prog, SEED, observed=[-np.inf, 0.0, 0.0, 0.0])
    assert r.eq[0] == np.isneginf(ref[:, 0, :]).sum() and r.gt[0] == r.total - r.eq[0]
    assert r.eq[2] == (ref[:, 2, :] == 0).sum() and r.nan[2] == np.isnan(ref[:, 2, :]).sum()     # (-0.0 ties with 0.0)


def test_ppc_over_the_stride_loop(demc, stride_twice):
    prog, chain, log_obj, ref = stride_twice
    r = demc.ppc_chain(chain, log_obj, prog, SEED, observed=[0.25])
    assert _counts(r) == _ref_counts(ref, [0.25]) and r.total == ref.shape[0] * ref.shape[2]
    assert 0 < r.gt[0] < r.total and r.p_value[0] == (r.gt[0] + r.eq[0]) / r.total


def test_ppc_engine_form_and_window_cuts(demc):
    N, d, K, G = 64, 3, 5, 40
    w = demc.workloads.mvnormal_problem(d, N)
    prog = demc.PredictiveProgram(pc.COUNT8, d, 2, names=["below", "sum"])
    e = _engine(demc, w, N, d, K, G, seed=61)
    e.run(1, G, w["gamma"])
    obs = [3.0, 4.0]
    r = e.ppc(prog, 11, 40, observed=obs)
    assert r.names == ["below", "sum"] and r.total == N * 30
    with e.predict(prog, 11, 40) as h:
        assert _counts(r) == _ref_counts(h.get(), obs)
    cut = e.ppc(prog, 11, 17, observed=obs) + e.ppc(prog, 18, 40, observed=obs)
    assert _counts(cut) == _counts(r) and cut.total == r.total
    assert _counts(e.ppc(prog, 11, 40, observed=obs, seed=61)) == _counts(r)
    assert _counts(e.ppc(prog, 11, 40, observed=obs, seed=62)) != _counts(r)
    e.close()


# ---- refusals: host-side checks that return before any launch ------------------------------------------------------------------
def test_refusals(demc):
    prog, _ = pc.generic_program(demc, 3, 2)
    chain, log_obj = _history(8, 4, 4, seed=1)
    with pytest.raises(ValueError):
        demc.predict_chain(chain, log_obj, prog, SEED)                # (the program's d is not the chain's)
    chain, log_obj = _history(8, 3, 4, seed=1)
    bad = demc.PredictiveProgram(pc.SYNTAX_ERROR, 3, 2)
    for call in (lambda: demc.predict_chain(chain, log_obj, bad, SEED), lambda: demc.ppc_chain(chain, log_obj, bad, SEED)):
        with pytest.raises(demc.DemczError) as ei:
            call()
        assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT and "program:4:" in str(ei.value)
    for call in (lambda: demc.predict_chain(chain, log_obj, prog, SEED, chain_id0=2**32 - 7),
                 lambda: demc.ppc_chain(chain, log_obj, prog, SEED, chain_id0=-1)):
        with pytest.raises(demc.DemczError) as ei:
            call()
        assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT and "2^32" in str(ei.value)
    with demc.predict_chain(chain, log_obj, prog, SEED) as h:
        second = demc.PredictiveProgram(pc.GENERIC, 2, 1)
        for bad_window in ((0, 3), (2, 5), (3, 2)):
            with pytest.raises(demc.DemczError) as ei:
                h.predict(second, *bad_window, seed=1)
            assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT
            with pytest.raises(demc.DemczError) as ei:
                h.ppc(second, *bad_window, seed=1)
            assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            h.predict(prog, 1, 4, seed=1)                             # (d = 3 against the derived history's 2 columns)
        with pytest.raises(demc.DemczError) as ei:
            h.predict(demc.PredictiveProgram(pc.SYNTAX_ERROR, 2, 2), 1, 4, seed=1)
        assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT and "program:4:" in str(ei.value)


# ---- the statistics over a predicted history ------------------------------------------------------------------------------------
def test_predicted_history_takes_the_statistics(demc):
    prog = demc.PredictiveProgram(pc.GENERIC, 3, 3, names=["a", "b", "c"])
    chain, log_obj = _history(64, 3, 40, seed=71)
    with demc.predict_chain(chain, log_obj, prog, SEED) as h:
        v = h.get()
        s = h.summary(PROBS, hdi_prob=0.9)
        ref = demc.posterior_summary(v, probs=PROBS, hdi_prob=0.9)
        assert set(s) == set(ref) | {"names"} and s["names"] == ["a", "b", "c"]
        assert np.array_equal(s["quantiles"], ref["quantiles"]) and np.array_equal(s["hdi"], ref["hdi"])
        for k in ("mean", "sd", "mcse", "ess", "rhat"):
            assert np.allclose(s[k], ref[k], rtol=1e-9, atol=0), k
        assert np.array_equal(h.quantiles(5, 30, PROBS), demc.quantile_chain(np.asfortranarray(v[:, :, 4:30]), PROBS))
        assert np.array_equal(h.hdi(5, 30, 0.8), demc.hdi_chain(np.asfortranarray(v[:, :, 4:30]), 0.8))
        # the MCSE of a p-value: predict -> indicator_le -> ess
        with h.indicator_le(1, 40, [0.0, 0.0, 0.0]) as ind:
            p = 1.0 - ind.mean_cov(1, 40)[0]
            assert np.allclose(p, (v > 0.0).mean(axis=(0, 2)), rtol=1e-12, atol=0)
            assert np.all(ind.ess(1, 40).ess > 0)
