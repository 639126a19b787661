"""Program targets (DEMCZ_TARGET_PROGRAM) on the device: a log-density written as HIP C++, compiled at run time with hipRTC into
window_kernel<TARGET_PROGRAM, d, FULL>.  Restatements of the built-in targets must reproduce the oracle and the committed goldens
(bit for bit, or at the NumPy restatement's stated tolerances); a target with no built-in (Rosenbrock) must reproduce the
host-closure path, whose Python closure performs the same IEEE operations in the same order (Python floats do not fuse, and the
program is compiled with contraction off)."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib
from helpers import oracle_sample

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
TOL = dict(rtol=1e-10, atol=1e-13)          # tests/test_numpy_restatement.py: trajectories over <= 60 generations

ISO = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) {
        const double r = x[i] - data[i];
        q = (i == 0) ? r * r : fma(r, r, q);
    }
    return -q;
}
"""

# data = mu (d) || W packed row-major lower triangle (row i at i(i+1)/2) || c0: the order of target_logp's full-block MvNormal
MVN = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const double* W = data + DEMCZ_D;
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) {
        const double* wrow = W + (i * (i + 1)) / 2;
        double acc = wrow[0] * (x[0] - data[0]);
        for (int j = 1; j <= i; ++j) acc = fma(wrow[j], x[j] - data[j], acc);
        q = (i == 0) ? acc * acc : fma(acc, acc, q);
    }
    return fma(-0.5, q, data[DEMCZ_D + (DEMCZ_D * (DEMCZ_D + 1)) / 2]);
}
"""

# data = design (nobs x d, row-major) || y: the regression SSE in the spec's sixteen interleaved partial sums and fixed tree
LINREG = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int64_t nobs = ndata / (DEMCZ_D + 1);
    const double* y = data + nobs * DEMCZ_D;
    double part[16];
    for (int l = 0; l < 16; ++l) part[l] = 0.0;
    const int64_t nfull = nobs / 16;
    for (int64_t k = 0; k < nfull; ++k) {
        for (int l = 0; l < 16; ++l) {
            const double* row = data + (k * 16 + l) * DEMCZ_D;
            double acc = row[0] * x[0];
            for (int j = 1; j < DEMCZ_D; ++j) acc = fma(row[j], x[j], acc);
            const double r = y[k * 16 + l] - acc;
            part[l] = (k == 0) ? r * r : fma(r, r, part[l]);
        }
    }
    for (int l = 0; l < 16; ++l) {
        const int64_t o = nfull * 16 + l;
        if (o < nobs) {
            const double* row = data + o * DEMCZ_D;
            double acc = row[0] * x[0];
            for (int j = 1; j < DEMCZ_D; ++j) acc = fma(row[j], x[j], acc);
            const double r = y[o] - acc;
            part[l] = (nfull == 0) ? r * r : fma(r, r, part[l]);
        }
    }
    for (int h = 8; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) part[l] = part[l] + part[l + h];
    return -0.5 * part[0];
}
"""

ROSENBROCK = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double s = 0.0;
    for (int i = 0; i + 1 < DEMCZ_D; ++i) {
        const double a = x[i + 1] - x[i] * x[i];
        const double b = 1.0 - x[i];
        s = s + 100.0 * (a * a) + b * b;
    }
    return -s;
}
"""

# data = design (nobs x d, row-major) || labels
LOGISTIC = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int64_t nobs = ndata / (DEMCZ_D + 1);
    const double* y = data + nobs * DEMCZ_D;
    double s = 0.0;
    for (int64_t o = 0; o < nobs; ++o) {
        double eta = 0.0;
        for (int j = 0; j < DEMCZ_D; ++j) eta = eta + data[o * DEMCZ_D + j] * x[j];
        s = s + (y[o] * eta - log1p(exp(eta)));
    }
    return s;
}
"""


def iso_program(mu):
    return demc.ProgramTarget(ISO, len(mu), data=mu)


def mvn_program(mu, W, c0):
    d = len(mu)
    wp = np.concatenate([np.asarray(W)[i, :i + 1] for i in range(d)])
    return demc.ProgramTarget(MVN, d, data=np.concatenate([mu, wp, [c0]]))


def linreg_program(design, y):
    design = np.asarray(design, dtype=np.float64)
    return demc.ProgramTarget(LINREG, design.shape[1], data=np.concatenate([np.ascontiguousarray(design).ravel(), y]))


def rosenbrock_closure(x):
    s = 0.0
    for i in range(len(x) - 1):
        a = x[i + 1] - x[i] * x[i]
        b = 1.0 - x[i]
        s = s + 100.0 * (a * a) + b * b
    return -s


def _same(mc, Z, ref):
    assert np.array_equal(mc.chain, ref["chain"]), "chain"
    assert np.array_equal(mc.log_obj, ref["log_obj"]), "log_obj"
    assert np.array_equal(mc.Xcurrent, ref["X"]), "Xcurrent"
    assert np.array_equal(Z, ref["Z"]), "Z"


# ---- 1. restated built-in targets against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("kind,N,d,blocks,tempered", [
    ("iso", 300, 10, None, False),
    ("iso", 300, 10, [[0, 1, 2, 3], [4, 5, 6, 7, 8, 9]], False),
    ("mvn", 300, 10, None, False),
    ("iso", 300, 10, None, True),
    ("mvn", 300, 10, None, True),
    ("mvn", 1024, 5, None, False),
    ("mvn", 1537, 5, None, False),
    ("iso", 1537, 5, [[4, 0], [1], [2, 3]], False),
])
def test_restated_builtin_equals_oracle(oracle, kind, N, d, blocks, tempered):
    K, G, seed = 5, 40, 20261016
    if kind == "iso":
        w = demc.workloads.iso_quad_problem(d, N)
        prog = iso_program(w["mu"])
    else:
        w = demc.workloads.mvnormal_problem(d, N)
        prog = mvn_program(w["target"].mu, w["target"].W, w["target"].c0)
    blocks = blocks or [list(range(d))]
    kw = dict(verbose=False, seed=seed)
    if tempered:
        T = np.array([demc.tempbaseline(g, G, 3, 1e-3) for g in range(1, G + 1)])
        mc, Z = demc.demcz_anneal(prog, w["Zinit"], N, K, G, len(blocks), blocks, w["eps_scale"], w["gamma"],
                                  temperaturefun=lambda ig, Ng, T0, TN: float(T[ig - 1]), adaptγ={"adapt": False}, **kw)
    else:
        T = None
        mc, Z = demc.demcz_sample(prog, w["Zinit"], N, K, G, len(blocks), blocks, w["eps_scale"], w["gamma"], **kw)
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, blocks, w["eps_scale"], w["gamma"], seed, temperature=T)
    _same(mc, Z, ref)


# ---- 2. restated targets against the committed goldens ---------------------------------------------------------------
def _golden_program(g):
    if "target_W" in g.files:
        return mvn_program(g["target_mu"], g["target_W"], float(g["target_c0"]))
    if "target_Sigma" in g.files:
        t = demc.MvNormalTarget(g["target_mu"], g["target_Sigma"])
        return mvn_program(t.mu, t.W, t.c0)
    if "target_design" in g.files:
        return linreg_program(g["target_design"], g["target_y"])
    return iso_program(g["target_mu"])


def _golden_run(g, prog, blocks):
    N, K, G = int(g["N"]), int(g["K"]), int(g["G"])
    kw = dict(verbose=False, seed=int(g["seed"]))
    if g["temperature"].size == 0:
        return demc.demcz_sample(prog, g["Zinit"], N, K, G, len(blocks), blocks, g["eps_scale"], float(g["gamma"]), **kw)
    T = g["temperature"]
    return demc.demcz_anneal(prog, g["Zinit"], N, K, G, len(blocks), blocks, g["eps_scale"], float(g["gamma"]),
                             temperaturefun=lambda ig, Ng, T0, TN: float(T[ig - 1]), adaptγ={"adapt": False}, **kw)


@pytest.mark.parametrize("name", ["traj_isoquad_d10_anneal", "traj_mvn_d5_N4_sync", "traj_linreg_d10_anneal"])
def test_restated_targets_reproduce_oracle_goldens(name):
    g = np.load(GOLD / f"{name}.npz")
    offs, idx = g["block_offsets"], g["block_indices"]
    blocks = [[int(v) for v in idx[offs[i]:offs[i + 1]]] for i in range(len(offs) - 1)]
    mc, Z = _golden_run(g, _golden_program(g), blocks)
    assert np.array_equal(mc.chain, g["chain"]) and np.array_equal(mc.log_obj, g["log_obj"])
    assert np.array_equal(Z, g["Z"])


@pytest.mark.parametrize("name", ["np_traj_iso_d10_T0", "np_traj_iso_d30_anneal", "np_traj_mvn_d1", "np_traj_mvn_d3_K1",
                                  "np_traj_mvn_d12", "np_traj_mvn_d26_K5", "np_traj_linreg_d7_anneal"])
def test_restated_targets_match_numpy_restatement(name):
    g = np.load(GOLD / f"{name}.npz")
    offs, idx = g["block_offsets"], g["block_indices0"]
    blocks = [[int(v) for v in idx[offs[i]:offs[i + 1]]] for i in range(len(offs) - 1)]
    mc, Z = _golden_run(g, _golden_program(g), blocks)
    assert mc.chain.shape == g["chain"].shape and Z.shape == g["Z"].shape
    assert np.allclose(mc.chain, g["chain"], **TOL) and np.allclose(mc.log_obj, g["log_obj"], **TOL)
    assert np.allclose(Z, g["Z"], **TOL) and np.allclose(mc.Xcurrent, g["X"], **TOL)


# ---- 3. a target with no built-in, against the host-closure path -----------------------------------------------------
ROSEN_BLOCKS = {
    1: [[0]],
    7: [[0, 1, 2], [3], [6, 4], [5]],
    13: [[0, 1, 2, 3, 4, 5], [6], [9, 7, 8], [10], [11, 12]],
    32: [list(range(16)), [16], list(range(17, 31)), [31]],
}


@pytest.mark.parametrize("tempered", [False, True])
@pytest.mark.parametrize("d", [1, 7, 13, 32])
def test_rosenbrock_equals_host_closure(d, tempered):
    N, K, G, seed = 96, 5, 20, 77
    r = np.random.default_rng(d)
    Zinit = np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5)
    eps = 1e-3 * np.ones(d)
    runs = []
    for target in (demc.ProgramTarget(ROSENBROCK, d), rosenbrock_closure):
        for blocks in ([list(range(d))], ROSEN_BLOCKS[d]):
            kw = dict(verbose=False, seed=seed)
            if tempered:
                T = np.array([demc.tempbaseline(g, G, 10, 1e-2) for g in range(1, G + 1)])
                runs.append(demc.demcz_anneal(target, Zinit, N, K, G, len(blocks), blocks, eps, 0.8,
                                              temperaturefun=lambda ig, Ng, T0, TN: float(T[ig - 1]), adaptγ={"adapt": False}, **kw))
            else:
                runs.append(demc.demcz_sample(target, Zinit, N, K, G, len(blocks), blocks, eps, 0.8, **kw))
    for (a, Za), (b, Zb) in zip(runs[:2], runs[2:]):
        assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_obj, b.log_obj)
        assert np.array_equal(a.Xcurrent, b.Xcurrent) and np.array_equal(Za, Zb)
    assert np.count_nonzero(np.diff(runs[0][0].chain, axis=2)) > 0            # (proposals were accepted: the runs moved)


# ---- 4. transcendental functions: a logistic regression --------------------------------------------------------------
def test_logistic_regression_logp_matches_numpy():
    d, nobs, N, K, G, seed = 4, 50, 256, 5, 20, 5
    r = np.random.default_rng(11)
    design = 0.3 * r.standard_normal((nobs, d))
    labels = (r.random(nobs) < 0.5).astype(np.float64)
    prog = demc.ProgramTarget(LOGISTIC, d, data=np.concatenate([design.ravel(), labels]))
    Zinit = np.asfortranarray(r.standard_normal((max(10 * d, N), d)))
    eps = 1e-3 * np.ones(d)

    def np_logp(x):
        s = 0.0
        for o in range(nobs):
            eta = 0.0
            for j in range(d):
                eta = eta + design[o, j] * x[j]
            s = s + (labels[o] * eta - math.log1p(math.exp(eta)))
        return s

    mc, _ = demc.demcz_sample(prog, Zinit, N, K, G, 1, [range(d)], eps, 1.0, verbose=False, seed=seed)
    for gi in range(G):
        for c in range(N):
            assert math.isclose(mc.log_obj[c, gi], np_logp(mc.chain[c, :, gi]), rel_tol=1e-13, abs_tol=0.0), (c, gi)
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Zinit.shape[0] + N, Gcap=0, blockindex=[range(d)], eps_scale=eps, seed=seed,
                       target=prog)
    X0 = Zinit[-N:]
    e.set_state(X0, None, Zinit)
    _, lp0, _, _ = e.get_state(with_Z=False)
    e.close()
    for c in range(N):
        assert math.isclose(lp0[c], np_logp(X0[c]), rel_tol=1e-13, abs_tol=0.0), c


# ---- 5. autostop and sharding ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.5, 1e9])
def test_autostop_run_checked_equals_oracle(oracle, threshold):
    d, N, K, G, seed = 10, 256, 10, 60, 3
    w = demc.workloads.iso_quad_problem(d, N)
    opts = demc.demcopt(d, N=N, K=K, Ngeneration=G, eps_scale=w["eps_scale"], verbose=False, autostop="Rhat",
                        autostop_every=20, autostop_Rhat=threshold)
    mc, Z = demc.demcz_sample(iso_program(w["mu"]), w["Zinit"], opts, seed=seed)
    g_stop = mc.chain.shape[2]
    assert g_stop == (G if threshold < 1.0 else 20)          # (never below 0.5; always below 1e9: stops at the first check)
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, g_stop, [range(d)], w["eps_scale"], w["gamma"], seed)
    _same(mc, Z, ref)


def test_host_sharding_equals_one_handle():
    d, N, G = 7, 256, 45
    r = np.random.default_rng(4)
    Zinit = np.asfortranarray(0.5 * r.standard_normal((N, d)) + 0.5)
    opts = demc.demcopt(d, N=N, K=10, Ngeneration=G, eps_scale=1e-3 * np.ones(d), verbose=False, autostop="Rhat",
                        autostop_every=20, autostop_Rhat=1.0)
    prog = demc.ProgramTarget(ROSENBROCK, d)
    a, Za, ra = demc.demcz_sample(prog, Zinit, opts, seed=8, return_runner=True)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=2)
    b, Zb, rb = demc.demcz_sample(prog, Zinit, opts, seed=8, sharding=sh, return_runner=True)
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_obj, b.log_obj) and np.array_equal(Za, Zb)
    assert np.array_equal(ra.changed(1, G), rb.changed(1, G))
    ra.close(); rb.close()


# ---- 6. state and error paths (compile errors and host-side argument errors only) --------------------------------------
def _raw_handle(N, d, Mcap, Gcap, lanes=0, seed=1):
    L = _lib.load()
    offs = np.array([0, d], dtype=np.int32)
    idx = np.arange(d, dtype=np.int32)
    eps = 1e-5 * np.ones(d)
    cfg = _lib.Config()
    cfg.N, cfg.chain_id0, cfg.d, cfg.K, cfg.Mcap, cfg.Gcap, cfg.Nblocks = N, 0, d, 5, Mcap, Gcap, 1
    cfg.block_offsets, cfg.block_indices, cfg.eps_scale = _lib.ptr(offs, _lib._ip), _lib.ptr(idx, _lib._ip), _lib.ptr(eps)
    cfg.seed, cfg.device_id, cfg.target_kind, cfg.lanes_per_chain = seed, 0, _lib.TARGET_PROGRAM, lanes
    h = C.c_void_p()
    rc = L.demcz_create(C.byref(h), C.byref(cfg))
    return L, h, rc, eps


def test_set_state_before_set_program_is_a_state_error():
    d, N = 5, 64
    L, h, rc, _ = _raw_handle(N, d, 200, 10)
    assert rc == _lib.OK, L.demcz_last_error(None)
    try:
        X = np.asfortranarray(np.zeros((N, d)))
        Z = np.asfortranarray(np.random.default_rng(0).standard_normal((100, d)))
        assert L.demcz_set_state(h, _lib.ptr(X), None, _lib.ptr(Z), 100, 100) == _lib.ERR_STATE
        assert b"demcz_set_program" in L.demcz_last_error(h)
        assert L.demcz_run(h, 1, 5, 2.38, None) == _lib.ERR_STATE
    finally:
        L.demcz_destroy(h)


@pytest.mark.parametrize("lanes", [_lib.LAYOUT_SPLIT, _lib.LAYOUT_SPLIT_WAVE, 8])
def test_other_layouts_are_refused_at_create(lanes):
    L, h, rc, _ = _raw_handle(64, 5, 200, 10, lanes=lanes)
    if rc == _lib.OK:
        L.demcz_destroy(h)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert b"lanes_per_chain must be 0 or 1" in L.demcz_last_error(None)


def test_compile_error_then_corrected_program_on_the_same_handle(oracle):
    d, N, K, G, seed = 10, 128, 5, 20, 1
    w = demc.workloads.iso_quad_problem(d, N)
    Z0 = np.asfortranarray(w["Zinit"])
    M0 = Z0.shape[0]
    Mcap = M0 + -(-N * G // K)
    L, h, rc, _ = _raw_handle(N, d, Mcap, G, seed=seed)
    assert rc == _lib.OK, L.demcz_last_error(None)
    try:
        mu = np.ascontiguousarray(w["mu"])
        bad = ISO.replace("return -q;", "return -q + oops;")
        assert L.demcz_set_program(h, bad.encode(), None, _lib.ptr(mu), d) == _lib.ERR_INVALID_ARGUMENT
        assert b"oops" in L.demcz_last_error(h)
        assert L.demcz_set_program(h, ISO.encode(), b"", _lib.ptr(mu), d) == _lib.OK, L.demcz_last_error(h)
        assert L.demcz_set_program(h, ISO.encode(), b"", _lib.ptr(mu), d) == _lib.ERR_STATE          # once per handle
        eps = np.ascontiguousarray(w["eps_scale"])
        X = np.asfortranarray(Z0[M0 - N:])
        assert L.demcz_set_state(h, _lib.ptr(X), None, _lib.ptr(Z0), M0, M0) == _lib.OK, L.demcz_last_error(h)
        assert L.demcz_run(h, 1, G, w["gamma"], None) == _lib.OK, L.demcz_last_error(h)
        chain = np.zeros((N, d, G), order="F")
        lobj = np.zeros((N, G), order="F")
        assert L.demcz_get_history(h, 1, G, _lib.ptr(chain), _lib.ptr(lobj)) == _lib.OK
        buf = C.create_string_buffer(256)
        assert L.demcz_debug_kernel_name(h, buf, 256) == _lib.OK
        assert b"(program)" in buf.value
    finally:
        L.demcz_destroy(h)
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, [range(d)], eps, w["gamma"], seed)
    assert np.array_equal(chain, ref["chain"]) and np.array_equal(lobj, ref["log_obj"])


def test_engine_kernel_name_and_bad_program_raise():
    d, N = 7, 64
    e = demc.HipEngine(N=N, d=d, K=5, Mcap=200, Gcap=5, blockindex=[range(d)], eps_scale=1e-3 * np.ones(d), seed=1,
                       target=demc.ProgramTarget(ROSENBROCK, d))
    Z = np.asfortranarray(np.random.default_rng(1).standard_normal((100, d)))
    e.set_state(Z[-N:], None, Z)
    e.run(1, 5, 1.0)
    assert "(program)" in e.kernel_name() and "<4, 7, true>" in e.kernel_name()
    e.close()
    with pytest.raises(demc.DemczError) as ei:
        demc.HipEngine(N=N, d=d, K=5, Mcap=200, Gcap=5, blockindex=[range(d)], eps_scale=1e-3 * np.ones(d), seed=1,
                       target=demc.ProgramTarget(ROSENBROCK.replace("b * b", "b * bb"), d))
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT and "bb" in str(ei.value)
