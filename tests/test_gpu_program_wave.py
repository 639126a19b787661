"""Program targets on the wave-per-chain layout (lanes_per_chain = DEMCZ_LAYOUT_PROGRAM_WAVE) on the device: the user's
demcz_logobj compiled into window_kernel_ps (d = 2..5) / window_kernel_pw (d = 6..32), lane n of a chain's wavefront evaluating it
on candidate n of the pass's 31.  Everything is compared bit for bit (np.array_equal on the chain and log_obj histories, the
final population and its log-densities, the archive): restated built-in targets against the oracle, every program against the
one-lane program layout (and Rosenbrock against the host-closure path), through LIVE launches, one launch per K-window, ragged
workgroups, host-driven sharding and a forced hand-off time-out."""
import ctypes as C

import numpy as np
import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib
from helpers import oracle_sample
from program_texts import (ROSENBROCK, iso_program, linreg_program, logistic_program, mvn_program,
                           rosenbrock_closure)

pytestmark = pytest.mark.gpu

WAVE = _lib.LAYOUT_PROGRAM_WAVE
PS_MAX_N = 2048          # demcz_kernels_ps.h


def _temps(G):
    return np.array([demc.tempbaseline(g, G, 3, 1e-3) for g in range(1, G + 1)])


def _run(target, Zinit, N, K, G, eps, gamma, seed, lanes, T=None, calls=None, checked_every=0, before_run=None):
    """One handle, generations 1..G (in the given calls, or one; through demcz_run_checked when checked_every > 0).  Returns the five
    arrays and what the handle says about itself."""
    Zinit = np.asfortranarray(Zinit)
    d = Zinit.shape[1]
    M0 = Zinit.shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=eps, seed=seed,
                       target=target, lanes_per_chain=lanes)
    try:
        e.set_state(Zinit[-N:], None, Zinit)
        if before_run:
            before_run(e)
        if checked_every:
            g_stop, _, _ = e.run_checked(1, G, gamma, checked_every, 0.0, temperature=T)
            assert g_stop == G
        else:
            for a, b in (calls or [(1, G)]):
                e.run(a, b, gamma, temperature=None if T is None else T[a - 1:b])
            e.synchronize()
        chain, lobj = e.get_history(1, G)
        X, lp, Z, M = e.get_state()
        out = dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z), M=M, name=e.kernel_name(),
                   info=e.info(), live=e.live_status())
    finally:
        e.close()
    return out


def _same(a, b, what=""):
    for k in ("chain", "log_obj", "X", "logp", "Z"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def _wave_name(name, d):
    assert "(program)" in name and (("_ps<4," in name) if d <= 5 else ("_pw<4," in name)), name
    assert f"<4, {d}," in name, name


# ---- 4. restated built-ins against the oracle -------------------------------------------------------------------------------
def _builtin(kind, d, N):
    if kind == "iso":
        w = demc.workloads.iso_quad_problem(d, N)
        return w, iso_program(w["mu"])
    w = demc.workloads.mvnormal_problem(d, N)
    return w, mvn_program(w["target"].mu, w["target"].W, w["target"].c0)


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("N", [64, 300, 1024])
@pytest.mark.parametrize("d", [2, 3, 5, 6, 7, 10, 13, 20, 26, 32])
@pytest.mark.parametrize("kind", ["iso", "mvn"])
def test_restated_builtin_equals_oracle(oracle, kind, d, N, tempered):
    K, G, seed = 10, 60, 20261016
    w, prog = _builtin(kind, d, N)
    T = _temps(G) if tempered else None
    got = _run(prog, w["Zinit"], N, K, G, w["eps_scale"], w["gamma"], seed, WAVE, T=T)
    _wave_name(got["name"], d)
    assert got["info"]["lanes_per_chain"] == WAVE
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, None, w["eps_scale"], w["gamma"], seed, temperature=T)
    _same(got, ref, f"{kind} d={d} N={N}")


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("kind,d", [("mvn", 5), ("iso", 3), ("mvn", 20), ("iso", 7)])
def test_irregular_pass_lengths_equal_oracle(oracle, kind, d, tempered):
    """K = 7, G = 45 in calls that start and end off the boundaries: passes of 5 + 2, cut at boundaries and at a launch's end."""
    N, K, G, seed = 300, 7, 45, 5
    w, prog = _builtin(kind, d, N)
    T = _temps(G) if tempered else None
    got = _run(prog, w["Zinit"], N, K, G, w["eps_scale"], w["gamma"], seed, WAVE, T=T, calls=[(1, 3), (4, 23), (24, 45)])
    _wave_name(got["name"], d)
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, None, w["eps_scale"], w["gamma"], seed, temperature=T)
    _same(got, ref, f"{kind} d={d} K=7")


# ---- 5. the same program on both layouts ------------------------------------------------------------------------------------
def _user_program(name, d):
    """(program, Zinit maker, eps, gamma): programs with no built-in twin."""
    r = np.random.default_rng(100 + d)
    if name == "rosenbrock":
        return demc.ProgramTarget(ROSENBROCK, d), lambda N: 0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5, 1e-3, 0.8
    if name == "logistic":
        nobs = 200
        design = 0.3 * r.standard_normal((nobs, d))
        labels = (r.random(nobs) < 0.5).astype(np.float64)
        return logistic_program(design, labels), lambda N: r.standard_normal((max(10 * d, N), d)), 1e-3, 1.0
    nobs = 100
    design = np.ones((nobs, d))
    design[:, 1:] = r.standard_normal((nobs, d - 1))
    y = design @ (1.0 + 3.0 * r.random(d)) + r.standard_normal(nobs)
    return linreg_program(design, y), lambda N: r.standard_normal((max(10 * d, N), d)), 1e-5, 2.0


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("name,d", [("rosenbrock", 2), ("rosenbrock", 5), ("rosenbrock", 7), ("rosenbrock", 13), ("rosenbrock", 32),
                                    ("logistic", 4), ("logistic", 9), ("linreg", 6)])
def test_same_program_on_both_layouts(name, d, N, tempered):
    """One-lane layout against the wave layout, same seed: identical arrays.  LOGISTIC (200 observations) and LINREG (100; a
    dynamically indexed local array) bring loads of `data` and scratch traffic into the pass -- the vector-memory operations the
    kernel's counted waits do not count."""
    K, G, seed = 10, 60, 77
    prog, mkZ, eps, gamma = _user_program(name, d)
    Zinit = np.asfortranarray(mkZ(N))
    T = _temps(G) if tempered else None
    lane = _run(prog, Zinit, N, K, G, eps * np.ones(d), gamma, seed, 1, T=T)
    wave = _run(prog, Zinit, N, K, G, eps * np.ones(d), gamma, seed, WAVE, T=T)
    assert "(program)" in lane["name"] and "window_kernel<4," in lane["name"]
    _wave_name(wave["name"], d)
    _same(wave, lane, f"{name} d={d} N={N}")
    assert np.count_nonzero(np.diff(wave["chain"], axis=2)) > 0            # (proposals were accepted: the runs moved)


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("d", [2, 5, 7, 13, 32])
def test_rosenbrock_wave_equals_host_closure(d, tempered):
    N, K, G, seed = 256, 10, 60, 77
    r = np.random.default_rng(d)
    Zinit = np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5)
    eps = 1e-3 * np.ones(d)
    T = _temps(G) if tempered else None
    runs = []
    for target, lanes in ((demc.ProgramTarget(ROSENBROCK, d), WAVE), (rosenbrock_closure, 0)):
        kw = dict(verbose=False, seed=seed, lanes_per_chain=lanes)
        if tempered:
            runs.append(demc.demcz_anneal(target, Zinit, N, K, G, 1, [range(d)], eps, 0.8,
                                          temperaturefun=lambda ig, Ng, T0, TN: float(T[ig - 1]), adaptγ={"adapt": False}, **kw))
        else:
            runs.append(demc.demcz_sample(target, Zinit, N, K, G, 1, [range(d)], eps, 0.8, **kw))
    (a, Za), (b, Zb) = runs
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_obj, b.log_obj)
    assert np.array_equal(a.Xcurrent, b.Xcurrent) and np.array_equal(a.log_objcurrent, b.log_objcurrent) and np.array_equal(Za, Zb)


# ---- 6. a long LIVE run ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rosenbrock5", "mvn20"])
def test_long_live_run_through_run_checked(oracle, which):
    """2000 generations through demcz_run_checked, the R-hat check per 1000-generation slab: a LIVE launch spans a slab."""
    N, K, G, seed = 1024, 10, 2000, 9
    if which == "mvn20":
        w, prog = _builtin("mvn", 20, N)
        Zinit, eps, gamma = w["Zinit"], w["eps_scale"], w["gamma"]
    else:
        prog, mkZ, e1, gamma = _user_program("rosenbrock", 5)
        Zinit, eps = np.asfortranarray(mkZ(N)), e1 * np.ones(5)
    lane = _run(prog, Zinit, N, K, G, eps, gamma, seed, 1, checked_every=1000)
    wave = _run(prog, Zinit, N, K, G, eps, gamma, seed, WAVE, checked_every=1000)
    _wave_name(wave["name"], prog.d)
    _same(wave, lane, which)
    on, redos = wave["live"]
    print(f"{which}: LIVE {on}, redos {redos}, window launches wave {wave['info']['window_launches']} / one lane {lane['info']['window_launches']}")
    assert on and redos == 0
    assert lane["info"]["window_launches"] >= G // K
    assert wave["info"]["window_launches"] * 10 <= lane["info"]["window_launches"]
    if which == "mvn20":
        ref = oracle_sample(oracle, w["target"], Zinit, N, K, G, None, eps, gamma, seed)
        _same(wave, ref, "mvn20 against the oracle")


# ---- 7. fall-backs and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,live", [(1537, False), (301, True)])
def test_ragged_and_oversized_populations(N, live):
    """N = 1537: not a multiple of a workgroup's four chains and more than a LIVE launch holds (one launch per K-window);
    N = 301: LIVE, ragged last workgroup."""
    d, K, G, seed = 5, 10, 60, 3
    prog, mkZ, e1, gamma = _user_program("rosenbrock", d)
    Zinit = np.asfortranarray(mkZ(N))
    lane = _run(prog, Zinit, N, K, G, e1 * np.ones(d), gamma, seed, 1)
    wave = _run(prog, Zinit, N, K, G, e1 * np.ones(d), gamma, seed, WAVE)
    _wave_name(wave["name"], d)
    _same(wave, lane, f"N={N}")
    assert wave["live"][0] == live and wave["live"][1] == 0
    if not live:
        assert wave["info"]["window_launches"] >= G // K and ", false," in wave["name"]


def _raw_create(N, d, blocks, lanes, kind, Mcap=4096):
    L = _lib.load()
    offs = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int32)
    idx = np.array([i for b in blocks for i in b], dtype=np.int32)
    eps = 1e-5 * np.ones(d)
    mu = np.zeros(d)
    W = np.asfortranarray(np.eye(d))
    cfg = _lib.Config()
    cfg.N, cfg.chain_id0, cfg.d, cfg.K, cfg.Mcap, cfg.Gcap, cfg.Nblocks = N, 0, d, 5, Mcap, 10, len(blocks)
    cfg.block_offsets, cfg.block_indices, cfg.eps_scale = _lib.ptr(offs, _lib._ip), _lib.ptr(idx, _lib._ip), _lib.ptr(eps)
    cfg.seed, cfg.device_id, cfg.target_kind, cfg.lanes_per_chain = 1, 0, kind, lanes
    cfg.mu, cfg.W = _lib.ptr(mu), _lib.ptr(W)
    h = C.c_void_p()
    rc = L.demcz_create(C.byref(h), C.byref(cfg))
    msg = (L.demcz_last_error(None) or b"").decode()
    if rc == _lib.OK:
        L.demcz_destroy(h)
    return rc, msg


@pytest.mark.parametrize("case,words", [
    ("blocks", "one block 0..d-1 in order"),
    ("permuted", "one block 0..d-1 in order"),
    ("d1", "2 <= d <= 32"),
    ("bigN", "N <= 2048"),
    ("builtin", "target_kind must be DEMCZ_TARGET_PROGRAM"),
    ("archive", "32-bit offsets"),
])
def test_refusals_at_create(case, words):
    N, d, blocks, kind, Mcap = 64, 5, [[0, 1, 2, 3, 4]], _lib.TARGET_PROGRAM, 4096
    if case == "blocks":
        blocks = [[0, 1], [2, 3, 4]]
    elif case == "permuted":
        blocks = [[1, 0, 2, 3, 4]]
    elif case == "d1":
        d, blocks = 1, [[0]]
    elif case == "bigN":
        N = PS_MAX_N + 1
    elif case == "builtin":
        kind = _lib.TARGET_MVNORMAL
    elif case == "archive":
        Mcap = 2**32 // 64 + 1          # (rows of 8 doubles: one past what 32-bit byte offsets reach; nothing is allocated)
    rc, msg = _raw_create(N, d, blocks, WAVE, kind, Mcap)
    assert rc == _lib.ERR_INVALID_ARGUMENT, msg
    assert words in msg, msg


def test_comm_init_and_peer_group_are_state_errors():
    d, N = 5, 64
    mk = lambda c0: demc.HipEngine(N=N, d=d, K=5, Mcap=400, Gcap=5, blockindex=[range(d)], eps_scale=1e-3 * np.ones(d), seed=1,
                                   target=demc.ProgramTarget(ROSENBROCK, d), chain_id0=c0, lanes_per_chain=WAVE)
    a, b = mk(0), mk(N)
    try:
        uid = a.comm_unique_id()
        with pytest.raises(demc.DemczError) as ei:
            a.comm_init(uid, 1, 0)
        assert ei.value.code == _lib.ERR_STATE and "DEMCZ_LAYOUT_PROGRAM_WAVE" in str(ei.value)
        with pytest.raises(demc.DemczError) as ei:
            demc.HipEngine.peer_group([a, b])
        assert ei.value.code == _lib.ERR_STATE and "DEMCZ_LAYOUT_PROGRAM_WAVE" in str(ei.value)
    finally:
        a.close(); b.close()


def test_host_sharding_equals_one_handle():
    """1024 chains over two handles whose rows the host appends (one launch per K-window on the wave kernel) = one handle."""
    d, N, G = 7, 1024, 45
    r = np.random.default_rng(4)
    Zinit = np.asfortranarray(0.5 * r.standard_normal((N, d)) + 0.5)
    opts = demc.demcopt(d, N=N, K=10, Ngeneration=G, eps_scale=1e-3 * np.ones(d), verbose=False, autostop="Rhat",
                        autostop_every=20, autostop_Rhat=1.0)
    prog = demc.ProgramTarget(ROSENBROCK, d)
    a, Za, ra = demc.demcz_sample(prog, Zinit, opts, seed=8, lanes_per_chain=WAVE, return_runner=True)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=2)
    b, Zb, rb = demc.demcz_sample(prog, Zinit, opts, seed=8, lanes_per_chain=WAVE, sharding=sh, return_runner=True)
    c, Zc = demc.demcz_sample(prog, Zinit, opts, seed=8, lanes_per_chain=1)
    try:
        assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_obj, b.log_obj) and np.array_equal(Za, Zb)
        assert np.array_equal(a.Xcurrent, b.Xcurrent) and np.array_equal(a.log_objcurrent, b.log_objcurrent)
        assert np.array_equal(ra.changed(1, G), rb.changed(1, G))
        assert np.array_equal(a.chain, c.chain) and np.array_equal(a.log_obj, c.log_obj) and np.array_equal(Za, Zc)
    finally:
        ra.close(); rb.close()


# ---- 8. a forced hand-off time-out -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polls", [1, -1])
def test_forced_handoff_timeout_is_redone(polls):
    """demcz_debug_set_live_fault late in a 1000-generation demcz_run_checked call (launches that start at generation 801 or later
    get a poll limit of 1, or find the error word pre-set: their waves leave early): the call is redone with one launch per
    K-window, the handle reports one redo, and the result is the one-lane layout's."""
    d, N, K, G, seed = 5, 512, 2, 1000, 21
    prog, mkZ, e1, gamma = _user_program("rosenbrock", d)
    Zinit = np.asfortranarray(mkZ(N))
    lane = _run(prog, Zinit, N, K, G, e1 * np.ones(d), gamma, seed, 1, checked_every=200)
    wave = _run(prog, Zinit, N, K, G, e1 * np.ones(d), gamma, seed, WAVE, checked_every=200,
                before_run=lambda e: (e.set_live_rearms(0), e.debug_set_live_fault(polls, 801)))
    _wave_name(wave["name"], d)
    on, redos = wave["live"]
    assert redos == 1, wave["live"]
    _same(wave, lane, f"polls={polls}")
