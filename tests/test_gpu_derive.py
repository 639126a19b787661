"""GPU: derived quantities (demcz_derive, demcz_kernels_derive.h) -- user functions of the draws evaluated on the device into a
derived history, against the NumPy restatements of tests/derive_cases.py: bit for bit where the program is +, -, *, comparisons
and selects, at derive_cases.REL_TOL where it calls exp / log1p / sqrt / divides.  Shapes are the smallest at which the kernel
can go wrong: one draw, a wave across a generation boundary, both limits, a ragged workgroup, a second ragged pass of the stride
loop.  Every refusal below is a host-side check that returns before any launch."""
import math

import numpy as np
import pytest

import derive_cases as dc
from helpers import bits_differ

pytestmark = pytest.mark.gpu

PROBS = [0.05, 0.5, 0.95]


def _engine(demc, w, N, d, K, G, seed, Gcap=None, chain_id0=0, lanes=0):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G if Gcap is None else Gcap, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=seed, target=w["target"], chain_id0=chain_id0, lanes_per_chain=lanes)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


def _derive_array(demc, prog, chain, log_obj):
    with demc.derive_chain(chain, log_obj, prog) as h:
        return h.get()


# ---- array form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,G,m", [(1, 1, 1, 1), (70, 3, 5, 2), (64, 32, 3, 32), (257, 5, 9, 3)])
def test_array_form_is_the_restatement_bit_for_bit(demc, N, d, G, m):
    prog, f = dc.generic_program(demc, d, m)
    chain, log_obj = dc.history(N, d, G, seed=100 + N)
    got = _derive_array(demc, prog, chain, log_obj)
    assert got.shape == (N, m, G) and got.flags.f_contiguous
    assert np.array_equal(got, f(chain, log_obj))


def test_stride_loop_runs_twice_with_a_ragged_last_pass(demc):
    threads, max_wg = demc._lib.derive_launch_constants()
    cap = threads * max_wg                       # lanes of the largest launch: a window of more draws is strided over
    N, d, m = 1031, 2, 1
    G = cap // N + 2
    total = N * G
    assert cap < total < 2 * cap and (total - cap) % cap != 0 and (total - cap) % threads != 0
    prog, f = dc.generic_program(demc, d, m)
    chain, log_obj = dc.history(N, d, G, seed=5)
    got = _derive_array(demc, prog, chain, log_obj)
    assert np.array_equal(got, f(chain, log_obj))


def test_non_finite_inputs_keep_their_bits(demc):
    N, d, G, m = 70, 3, 5, 3
    prog, f = dc.generic_program(demc, d, m)
    chain, log_obj = dc.history(N, d, G, seed=8)
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e308, -1e308, 5e-324]
    r = np.random.default_rng(9)
    for i, v in enumerate(specials * 4):
        chain[r.integers(N), i % d, r.integers(G)] = v
    for i, v in enumerate(specials):
        log_obj[r.integers(N), r.integers(G)] = v
    chain[0, 0, 0], chain[1, 0, 0], chain[2, 0, 0] = -0.0, np.nan, -np.inf      # (the select's operand too)
    got = _derive_array(demc, prog, chain, log_obj)
    why = bits_differ(got, f(chain, log_obj))
    assert why is None, why
    assert np.isnan(got).any() and np.isinf(got).any()


def test_without_log_obj_logp_is_nan(demc):
    N, d, G, m = 70, 3, 5, 3
    prog, f = dc.generic_program(demc, d, m)
    chain, _ = dc.history(N, d, G, seed=12)
    got = _derive_array(demc, prog, chain, None)
    assert np.isnan(got[:, 2, :]).all()                       # (column 2 subtracts logp)
    assert np.array_equal(got[:, :2, :], f(chain, None)[:, :2, :])


def test_unwritten_outputs_stay_nan(demc):
    prog, f = dc.program(demc, "first_only")
    chain, log_obj = dc.history(130, prog.d, 3, seed=13)
    got = _derive_array(demc, prog, chain, log_obj)
    assert np.isnan(got[:, 1:, :]).all()
    assert np.array_equal(got[:, 0, :], f(chain, log_obj)[:, 0, :])


def test_data_reaches_the_program(demc):
    with_data, f = dc.program(demc, "with_data")
    constants, _ = dc.program(demc, "with_constants")
    chain, log_obj = dc.history(130, with_data.d, 4, seed=14)
    a = _derive_array(demc, with_data, chain, log_obj)
    b = _derive_array(demc, constants, chain, log_obj)        # (no data: its `data` pointer is NULL, which column 2 reports)
    assert np.array_equal(a, b) and np.array_equal(a, f(chain, log_obj))


def test_transcendental_program_at_the_device_tolerance(demc):
    prog, f = dc.program(demc, "transcendental")
    chain, log_obj = dc.history(70, prog.d, 5, seed=15)
    got = _derive_array(demc, prog, chain, log_obj)
    ref = f(chain, log_obj)
    worst = 0.0
    for a, b in zip(got.ravel(), ref.ravel()):
        worst = max(worst, abs(a - b) / abs(b))
        assert math.isclose(a, b, rel_tol=dc.REL_TOL, abs_tol=0.0), (a, b)
    print(f"[derive] transcendental: worst relative difference {worst:.3e}")


def test_derive_of_a_derive(demc):
    first, f1 = dc.generic_program(demc, 4, 3)
    second, f2 = dc.program(demc, "second")
    chain, log_obj = dc.history(70, 4, 6, seed=16)
    with demc.derive_chain(chain, log_obj, first) as h1:
        h2 = h1.derive(second, 2, 5)
    got = h2.get()                                            # (h1 is closed: a derived history owns its memory)
    assert (h2.g_from, h2.g_to) == (2, 5)
    h2.close()
    ref = f2(f1(chain, log_obj)[:, :, 1:5], None)
    assert np.array_equal(got, ref)
    assert np.all(got[:, 1, :] == 0.0)                        # logp of a derived history is NaN


def test_program_dimension_must_be_the_history_s(demc):
    prog, _ = dc.generic_program(demc, 3, 2)
    chain, log_obj = dc.history(8, 4, 4, seed=1)
    with pytest.raises(ValueError):
        demc.derive_chain(chain, log_obj, prog)


def test_compile_error_in_the_array_form_carries_the_log(demc):
    chain, log_obj = dc.history(8, 3, 4, seed=1)
    with pytest.raises(demc.DemczError) as ei:
        demc.derive_chain(chain, log_obj, demc.DerivedProgram(dc.SYNTAX_ERROR, 3, 2))
    assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT and "program:4:" in str(ei.value)


# ---- engine form --------------------------------------------------------------------------------------------------------------
def test_engine_form_reads_the_right_slots_and_log_obj(demc):
    N, d, K, G = 64, 3, 5, 40
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = dc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, K, G, seed=21)
    e.run(1, G, w["gamma"])
    h = e.derive(prog, 11, 40)
    assert (h.N, h.m, h.g_from, h.g_to) == (N, 3, 11, 40)
    assert np.array_equal(h.get(), f(*e.get_history(11, 40)))
    assert np.array_equal(h.get(20, 25), f(*e.get_history(20, 25)))
    for bad in ((30, 41), (0, 10), (12, 11)):
        with pytest.raises(demc.DemczError) as ei:
            e.derive(prog, *bad)
        assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT
    with pytest.raises(demc.DemczError) as ei:
        e.derive(demc.DerivedProgram(dc.SYNTAX_ERROR, d, 2), 11, 40)
    assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT and "program:4:" in str(ei.value)
    ref = f(*e.get_history(11, 40))
    e.close()
    assert np.array_equal(h.get(), ref)                       # the derived history survives its source
    assert np.all(np.isfinite(h.rhat(11, 40)))
    h.close()
    h.close()                                                 # (idempotent)


def test_engine_form_after_the_history_origin_moved(demc):
    N, d, K = 64, 3, 5
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = dc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, K, 60, seed=22, Gcap=30)
    e.run(1, 30, w["gamma"])
    e.synchronize()
    e.set_history_origin(30)
    e.run(31, 60, w["gamma"])
    with e.derive(prog, 36, 57) as h:
        assert np.array_equal(h.get(), f(*e.get_history(36, 57)))
        assert np.array_equal(h.quantiles(40, 50, PROBS), demc.quantile_chain(h.get(40, 50), PROBS))
    with pytest.raises(demc.DemczError) as ei:
        e.derive(prog, 25, 40)                                # (generations 25..30 left the window)
    assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT
    e.close()


def test_engine_without_history_is_a_state_error(demc):
    N, d = 64, 3
    w = demc.workloads.mvnormal_problem(d, N)
    prog, _ = dc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, 5, 20, seed=23, Gcap=0)
    e.run(1, 20, w["gamma"])
    with pytest.raises(demc.DemczError) as ei:
        e.derive(prog, 1, 20)
    assert ei.value.code == demc._lib.ERR_STATE
    e.close()


def test_after_live_launches(demc):
    """N = 256, d = 5, K = 2: the shape at which tests/test_gpu_live.py sees LIVE launches inside demcz_run_checked.  The last
    demcz_run is not synchronised: demcz_derive verifies it (live_verify) before it reads the history."""
    N, d, K, G, every = 256, 5, 2, 400, 100
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = dc.generic_program(demc, d, 3)
    e = _engine(demc, w, N, d, K, G, seed=43)
    e.run_checked(1, 300, w["gamma"], every, 0.0)
    e.run(301, G, w["gamma"])
    h = e.derive(prog, 101, G)
    assert e.live_status()[0], "this shape is expected to run LIVE launches"
    assert np.array_equal(h.get(), f(*e.get_history(101, G)))
    h.close()
    e.close()


# ---- the statistics over a derived history ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def derived(demc):
    N, d, K, G = 64, 3, 5, 50
    w = demc.workloads.mvnormal_problem(d, N)
    prog = demc.DerivedProgram(dc.GENERIC, d, 3, names=["sum", "signed", "minus_logp"])
    e = _engine(demc, w, N, d, K, G, seed=31)
    e.run(1, G, w["gamma"])
    h = e.derive(prog, 11, 50)
    e.close()
    yield h, h.get()
    h.close()


def test_statistics_are_those_of_the_values(demc, derived):
    h, v = derived
    assert v.shape == (64, 3, 40)
    tol = dict(rtol=1e-9, atol=0)
    for a, b in ((11, 50), (15, 46)):                         # the whole window, and one inside: generations keep their numbers
        sub = np.asfortranarray(v[:, :, a - 11:b - 11 + 1])
        assert np.array_equal(h.quantiles(a, b, PROBS), demc.quantile_chain(sub, PROBS))
        assert np.allclose(h.rhat(a, b), demc.Rhat_gelman(sub), **tol)
        assert np.allclose(h.ess(a, b).ess, demc.ess_chain(sub).ess, **tol)
        mean, cov = h.mean_cov(a, b)
        rm, rc = demc.mean_cov_chain(sub)
        assert np.allclose(mean, rm, **tol) and np.allclose(cov, rc, rtol=1e-9, atol=1e-18)
    with pytest.raises(demc.DemczError) as ei:
        h.rhat(1, 40)                                         # (generations 1..10 are not in it)
    assert ei.value.code == demc._lib.ERR_INVALID_ARGUMENT


def test_summary_has_the_keys_of_posterior_summary(demc, derived):
    h, v = derived
    s = h.summary(PROBS)
    ref = demc.posterior_summary(v, probs=PROBS)
    assert set(s) == set(ref) | {"names"} and s["names"] == ["sum", "signed", "minus_logp"]
    assert np.array_equal(s["quantiles"], ref["quantiles"])
    for k in ("mean", "sd", "mcse", "ess", "rhat"):
        assert np.allclose(s[k], ref[k], rtol=1e-9, atol=0), k
    assert set(h.summary()) == set(demc.posterior_summary(v)) | {"names"}


def test_what_a_derived_history_refuses(demc, derived):
    h, v = derived
    N = h.N
    other = demc.HipEngine
    calls = dict(
        run=lambda: other.run(h, 51, 52, 2.38),
        set_state=lambda: other.set_state(h, np.zeros((N, 3)), None, np.zeros((2 * N, 3))),
        get_state=lambda: other.get_state(h, with_Z=False),
        best=lambda: other.best(h, 11, 50),
        accept_ratio=lambda: other.accept_ratio(h, 11, 50),
        changed_total=lambda: other.changed_total(h, 11, 50),
        get_changed=lambda: other.get_changed(h, 11, 50),
        comm_init=lambda: other.comm_init(h, b"\0" * 128, 2, 0),
        peer_group=lambda: other.peer_group([h, h]),
        history_stream=lambda: other.history_stream(h, True),
        set_history_origin=lambda: other.set_history_origin(h, 5),
        run_checked=lambda: other.run_checked(h, 51, 60, 2.38, 5),
        propose=lambda: other.propose(h, 51, 0, 2.38),
        info=lambda: other.info(h),
    )
    for name, call in calls.items():
        with pytest.raises(demc.DemczError) as ei:
            call()
        assert ei.value.code == demc._lib.ERR_STATE, name
        assert "derived history" in str(ei.value), name
    # demcz_get_history with a log_obj pointer
    L, ch, lo = h._L, np.empty((N, 3, 40), order="F"), np.empty((N, 40), order="F")
    assert L.demcz_get_history(h._h, 11, 50, demc._lib.ptr(ch), demc._lib.ptr(lo)) == demc._lib.ERR_STATE
    assert L.demcz_get_history(h._h, 11, 50, demc._lib.ptr(ch), None) == demc._lib.OK and np.array_equal(ch, v)
    # ... and it still answers
    assert np.allclose(h.rhat(11, 50), demc.Rhat_gelman(v), rtol=1e-9, atol=0)
    h.synchronize()


# ---- shards -------------------------------------------------------------------------------------------------------------------
def test_host_sharding_equals_one_handle(demc):
    d, N, G = 3, 64, 40
    w = demc.workloads.mvnormal_problem(d, N)
    opts = demc.demcopt(d, N=N, K=5, Ngeneration=G, eps_scale=w["eps_scale"], verbose=False, autostop="Rhat", autostop_every=20,
                        autostop_Rhat=0.0)
    prog, f = dc.generic_program(demc, d, 3)
    a, Za, ra = demc.demcz_sample(w["target"], w["Zinit"], opts, seed=8, return_runner=True)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=2)
    b, Zb, rb = demc.demcz_sample(w["target"], w["Zinit"], opts, seed=8, sharding=sh, return_runner=True)
    assert [e.chain_id0 for e in rb.engines] == [0, 32] and len(ra.engines) == 1
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_obj, b.log_obj)
    with ra.derive(prog, 5, G) as da, rb.derive(prog, 5, G) as db:
        assert len(db.engines) == 2 and [h.N for h in db.engines] == [32, 32]
        va, vb = da.get(), db.get()
        assert np.array_equal(va, vb) and np.array_equal(va, f(a.chain[:, :, 4:], a.log_obj[:, 4:]))
        assert np.array_equal(da.quantiles(5, G, PROBS), db.quantiles(5, G, PROBS))
        assert np.array_equal(db.quantiles(5, G, PROBS), demc.quantile_chain(vb, PROBS))
        assert np.allclose(da.rhat(5, G), db.rhat(5, G), rtol=1e-9, atol=0)
        assert np.allclose(da.ess(5, G).ess, db.ess(5, G).ess, rtol=1e-9, atol=0)
    ra.close(); rb.close()


def test_members_of_a_replica_group(demc):
    """demcz_derive on handles that publish rows into each other's archives from inside their launches (demcz_peer_group): the
    call verifies the group's unverified launches first, then maps each member's own chains."""
    d, N, K, G = 5, 256, 10, 40
    w = demc.workloads.mvnormal_problem(d, N)
    prog, f = dc.generic_program(demc, d, 3)
    sh = demc.Sharding(mode="peer", local_shards=2)
    mc, Z, r = demc.demcz_sample(w["target"], w["Zinit"], N, K, G, 1, [range(d)], w["eps_scale"], w["gamma"], verbose=False,
                                 seed=12, sharding=sh, autostop="Rhat", autostop_Rhat=0.0, autostop_every=20, return_runner=True)
    with r.derive(prog, 1, G) as dr:
        v = dr.get()
        assert np.array_equal(v, f(mc.chain, mc.log_obj))
        assert np.array_equal(dr.quantiles(1, G, PROBS), demc.quantile_chain(v, PROBS))
    r.close()
