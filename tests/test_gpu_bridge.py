"""GPU: the marginal likelihood by bridge sampling on the device (demcz_bridge and its layers; K12 demcz_kernels_bridge.h) against
tests/bridge_reference.py.

  * the proposal's draws and a2 equal the reference bit for bit -- programs that write their fmas out and the built-in targets
    through a handle, d = 1, 2, 5, 7, 32 with 70 chains, and one launch long enough to reach the strided part of the loop;
  * a1 equals the reference bit for bit, a -inf and a NaN in log_obj passed through;
  * the iteration over every world of tests/bridge_cases.py: the reference's converged, n_nan and (where it converges) update
    count, NaN where it is NaN, values within bridge_reference's tolerances (printed before they are asserted), the same bits
    with one update and with four queued between synchronisations, and from two calls;
  * end to end on a history the CPU oracle reproduces: engine.bridge against the reference fed the returned proposal, the factor
    against demcz_mean_cov, bridge_chain of the downloaded arrays, a bounded-support program, a run with snooker generations
    and one on the wave-per-chain layout;
  * the refusals.

The refusal of a communicator with several ranks (the check demcz_rank_normalize makes, shared) needs two devices and is not run
here."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import bridge_cases as bc
import bridge_reference as br
import ess_reference as er
import oracle_py as O
import program_texts as pt
from demc_jl_amd import _lib
from helpers import bits_differ

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 5, 7, 32]
NP, WP, SEED = 70, 5, 4711


def same(a, b):
    d = bits_differ(a, b)
    assert d is None, d


def get(h):
    with h:
        return h.get()


@functools.lru_cache(maxsize=None)
def proposal_of(d):
    """(m, L) of a random well-conditioned proposal in d dimensions."""
    rng = np.random.default_rng(500 + d)
    A = rng.standard_normal((d, d))
    V = (A @ A.T / d + 0.5 * np.eye(d)) * 0.04
    return 0.3 + 0.1 * rng.standard_normal(d), np.asfortranarray(br.cholesky(V))


@functools.lru_cache(maxsize=None)
def reference_draws(d, Np=NP, wp=WP):
    """(x, logg) of the reference, computed once per shape and shared."""
    m, L = proposal_of(d)
    return br.proposal(SEED, Np, wp, m, L)


def targets_of(demc, d):
    """name -> (ProgramTarget or built-in target, oracle problem whose logp is its twin)"""
    w = demc.workloads.mvnormal_problem(d, 8)
    t = w["target"]
    iso = demc.IsoQuadTarget(w["mu"])
    prob = lambda tt: O.Problem(8, d, 10, 100, np.ones(d), 1, target=tt.spec())      # noqa: E731
    return dict(mvn_program=(pt.mvn_program(t.mu, t.W, t.c0), prob(t)), iso_program=(pt.iso_program(w["mu"]), prob(iso)),
                mvn_builtin=(t, prob(t)), iso_builtin=(iso, prob(iso)))


def check_proposal(a2h, xh, d, prob, Np=NP, wp=WP):
    x, logg = reference_draws(d, Np, wp)
    with np.errstate(all="ignore"):
        a2 = O.logp(prob, br.rows_of(x)).reshape(Np, wp) - logg
    got_x, got_a2 = get(xh), get(a2h)
    assert got_x.shape == (Np, d, wp) and got_a2.shape == (Np, 1, wp)
    same(got_x, x)
    same(got_a2[:, 0, :], a2)


# ---- the proposal layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_proposal_programs_bit_equal(demc, d):
    m, L = proposal_of(d)
    for name in ("mvn_program", "iso_program"):
        prog, prob = targets_of(demc, d)[name]
        a2h, xh = demc.bridge_proposal_program(prog, NP, WP, m, L, SEED, want_draws=True)
        check_proposal(a2h, xh, d, prob)
    # without the draws: the same a2
    prog, prob = targets_of(demc, d)["iso_program"]
    x, logg = reference_draws(d)
    same(get(demc.bridge_proposal_program(prog, NP, WP, m, L, SEED))[:, 0, :], O.logp(prob, br.rows_of(x)).reshape(NP, WP) - logg)


@pytest.mark.parametrize("d", DIMS)
def test_proposal_builtin_targets_bit_equal(demc, d):
    m, L = proposal_of(d)
    w = demc.workloads.mvnormal_problem(d, 8)
    for name in ("mvn_builtin", "iso_builtin"):
        target, prob = targets_of(demc, d)[name]
        e = demc.HipEngine(N=8, d=d, K=10, Mcap=w["Zinit"].shape[0] + 16, Gcap=4, blockindex=[range(d)], eps_scale=w["eps_scale"],
                           seed=3, target=target, lanes_per_chain=1)
        try:
            a2h, xh = e.bridge_proposal(NP, WP, m, L, seed=SEED, want_draws=True)
            check_proposal(a2h, xh, d, prob)
        finally:
            e.close()


def test_proposal_strided_launch(demc):
    """1031 x 520 = 536 120 draws > 2048 x 256 lanes: the second trip of the loop, with its carry from chain to generation."""
    d, Np, wp = 2, 1031, 520
    assert Np * wp > 2048 * 256
    m, L = proposal_of(d)
    prog, prob = targets_of(demc, d)["iso_program"]
    a2h, xh = demc.bridge_proposal_program(prog, Np, wp, m, L, SEED, want_draws=True)
    check_proposal(a2h, xh, d, prob, Np, wp)


# ---- the posterior layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_posterior_bit_equal(demc, d):
    N, w = 70, 9
    rng = np.random.default_rng(900 + d)
    m, L = proposal_of(d)
    chain = np.asfortranarray(m[None, :, None] + 0.3 * rng.standard_normal((N, d, w)))
    log_obj = np.asfortranarray(rng.standard_normal((N, w)) * 5.0 - 3.0)
    log_obj[3, 2], log_obj[69, 8] = -np.inf, np.nan
    want = br.posterior_a1(chain, log_obj, m, L)
    got = get(demc.bridge_posterior_chain(chain, log_obj, m, L))
    assert got.shape == (N, 1, w) and got[3, 0, 2] == -np.inf and np.isnan(got[69, 0, 8])
    same(got[:, 0, :], want)
    # the iteration window of the odd history (h = 4) on its own: the same values
    same(get(demc.bridge_posterior_chain(chain[:, :, 4:], log_obj[:, 4:], m, L))[:, 0, :], want[:, 4:])


# ---- the iteration --------------------------------------------------------------------------------------------------------------------
IDENTITY = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out) { out[0] = x[0]; }
"""


def upload(demc, a):
    """An N x w array as a one-column history on the device (the identity through demcz_derive_array; NaN and inf pass)."""
    a = np.asarray(a, dtype=np.float64)
    return demc.derive_chain(np.asfortranarray(a.reshape(a.shape[0], 1, a.shape[1])), None, demc.DerivedProgram(IDENTITY, 1, 1))


def iterate(demc, post, prop, args, batch):
    os.environ["DEMCZ_BRIDGE_BATCH"] = str(batch)
    try:
        return demc.bridge_iterate(post, prop, want_f2=True, **args)
    finally:
        del os.environ["DEMCZ_BRIDGE_BATCH"]


def same_iteration(a, b):
    assert (a.iterations, a.converged, a.n_nan) == (b.iterations, b.converged, b.n_nan)
    same([a.logml], [b.logml])
    same(a.moments, b.moments)


@pytest.mark.parametrize("i", range(len(bc.worlds())), ids=bc.names())
def test_iteration_worlds(demc, i):
    w, ref = bc.worlds()[i], bc.reference(i)
    with upload(demc, w["a1"]) as post, upload(demc, w["a2"]) as prop:
        r1 = iterate(demc, post, prop, w["args"], 1)
        r4 = iterate(demc, post, prop, w["args"], 4)
        r4b = iterate(demc, post, prop, w["args"], 4)
        same_iteration(r1, r4)
        same_iteration(r4, r4b)
        # (ESS of the device's own f2, before it is downloaded and freed)
        ess = None if w["nan"] else r4.f2.ess(r4.f2.g_from, r4.f2.g_to)
        f2 = [get(r.f2)[:, 0, :] for r in (r1, r4, r4b)]
        same(f2[0], f2[1])
        same(f2[1], f2[2])
        rd = demc.bridge_iterate(post, prop, **w["args"])              # the default batch, no f2
        assert rd.f2 is None
        same_iteration(rd, r4)
        assert r4.converged == ref["converged"] and r4.n_nan == ref["n_nan"]
        if w["nan"]:
            assert math.isnan(r4.logml) and np.all(np.isnan(r4.moments))
            return
        if w["converges"]:
            assert r4.iterations == ref["iterations"]
        else:
            assert r4.iterations == w["args"]["max_iter"]
        e = br.errors(dict(logml=r4.logml, moments=r4.moments), ref)
        ef2 = float(np.max(np.abs(f2[1].ravel(order="F") - ref["f2"]) / ref["f2"]))
        # se_logml with ONE ESS on both sides (the device's own, of the device's f2): the formula's tolerance
        se_ref_same = br.se_ext(ref["moments"], w["a2"].size, float(ess.ess[0]))
        ese = abs(demc.bridge_se(r4.moments, w["a2"].size, float(ess.ess[0])) - se_ref_same) / se_ref_same
        print(f"[bridge] {w['name']}: {r4.iterations} updates, logml {r4.logml:.6f} err {e['logml']:.2e} (tol {br.LOGML_TOL:.1e}), "
              f"moments {e['moments']:.2e} (tol {br.MOMENT_TOL:.1e}), se {ese:.2e} (tol {br.SE_TOL:.1e}), f2 {ef2:.2e} (tol {br.F2_TOL:.1e})")
        assert e["logml"] <= br.LOGML_TOL and e["moments"] <= br.MOMENT_TOL and ese <= br.SE_TOL and ef2 <= br.F2_TOL
        # ... and that ESS against the reference's, by demcz_ess's own tolerance
        _, _, margin = bc.reference_se(i)
        eref = br.ess_of_f2(ref["f2"], w["a1"].shape[0])[2]
        if margin >= er.MARGIN:
            assert abs(float(ess.tau[0]) - float(eref.tau[0])) <= er.TAU_ATOL_PER_LAG * (2 * int(eref.pairs[0]) + 1)


def test_iteration_windows_inside_the_histories(demc):
    """Windows that start inside either history give what the cut arrays give."""
    w = bc.worlds()[0]
    a1, a2 = w["a1"], w["a2"]
    with upload(demc, a1) as post, upload(demc, a2) as prop, upload(demc, a1[:, 10:140]) as pc, upload(demc, a2[:, 3:100]) as qc:
        a = demc.bridge_iterate(post, prop, g_from=11, g_to=140, gp_from=4, gp_to=100)
        b = demc.bridge_iterate(pc, qc)
        same_iteration(a, b)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def run_engine(demc, target, w, N, G, seed, **kw):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=w["d"], K=w["K"], Mcap=M0 + N * (G // w["K"] + 1), Gcap=G, blockindex=[range(w["d"])],
                       eps_scale=w["eps_scale"], seed=seed, target=target, **kw)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


@pytest.fixture(scope="module")
def e2e(demc):
    w, prob, chain, log_obj = bc.oracle_history()
    t = w["target"]
    prog = pt.mvn_program(t.mu, t.W, t.c0)
    e = run_engine(demc, prog, w, bc.E2E["N"], bc.E2E["G"], bc.E2E["seed"])
    e.run(1, bc.E2E["G"], w["gamma"])
    yield e, prog, prob, chain, log_obj
    e.close()


def test_end_to_end_against_the_reference(demc, e2e):
    e, prog, prob, chain, log_obj = e2e
    a, b = bc.E2E["window"]
    gc, gl = e.get_history(1, bc.E2E["G"])
    same(gc, chain)
    same(gl, log_obj)
    r = e.bridge(a, b)
    hw = (b - a + 1) // 2
    assert r.converged and r.n_nan == 0 and r.n_post == r.n_prop == bc.E2E["N"] * (b - a + 1 - hw)
    assert r.neff == float(np.median(e.ess(a + hw, b).ess))
    # the proposal: demcz_mean_cov of the fit window and its factor
    m, V = e.mean_cov(a, a + hw - 1)
    same(r.mean, m)
    ce = br.cholesky_error(r.L, V)
    print(f"[bridge] end to end: |L L^T - V| {ce:.2e} (tol {br.CHOL_TOL:.1e})")
    assert ce <= br.CHOL_TOL and np.all(np.triu(r.L, 1) == 0.0)
    same(r.L, br.cholesky(V))
    # the reference fed the returned m and L: both sides bit for bit, then the iteration in the wide numbers
    seed = demc.bridge_seed(bc.E2E["seed"])
    ref = br.bridge_f64(chain[:, :, a - 1:b], log_obj[:, a - 1:b], lambda x: O.logp(prob, x), seed=seed, neff=r.neff, fma=br.fma,
                        m=r.mean, L=r.L)
    same(get(e.bridge_posterior(a + hw, b, r.mean, r.L))[:, 0, :], ref["a1"])
    same(get(e.bridge_proposal(bc.E2E["N"], b - a + 1 - hw, r.mean, r.L))[:, 0, :], ref["a2"])
    ext = br.iterate_ext(ref["a1"], ref["a2"], neff=r.neff)
    err = br.errors(dict(logml=r.logml, moments=ext["moments"]), ext)["logml"]
    se_same = br.se_ext(ext["moments"], r.n_prop, r.ess_f2)
    ese = abs(r.se_logml - se_same) / se_same
    eref = br.ess_of_f2(ext["f2"], bc.E2E["N"])[2]
    print(f"[bridge] end to end: logml {r.logml:.6f} se {r.se_logml:.4f} ({r.iterations} updates) err {err:.2e} (tol {br.LOGML_TOL:.1e}), "
          f"se err {ese:.2e} (tol {br.SE_TOL:.1e}), ESS(f2) {r.ess_f2:.1f} against {float(eref.ess[0]):.1f}")
    assert r.iterations == ext["iterations"] and err <= br.LOGML_TOL and ese <= br.SE_TOL
    if float(eref.margin[0]) >= er.MARGIN:
        tau = r.n_post / r.ess_f2
        assert abs(tau - float(eref.tau[0])) <= er.TAU_ATOL_PER_LAG * (2 * int(eref.pairs[0]) + 1) * 1.0001
    assert abs(r.logml) <= br.GUARD_Z * r.se_logml                        # (the target is a normalised density: log Z = 0)
    # the host-array form on the downloaded window: the same bits; neff given and None
    rc = demc.bridge_chain(chain[:, :, a - 1:b], log_obj[:, a - 1:b], prog, seed=seed, neff=r.neff)
    for f in ("logml", "se_logml", "neff", "ess_f2"):
        same([getattr(rc, f)], [getattr(r, f)])
    assert (rc.iterations, rc.converged, rc.n_post, rc.n_prop, rc.n_nan) == (r.iterations, r.converged, r.n_post, r.n_prop, r.n_nan)
    same(rc.mean, r.mean)
    same(rc.L, r.L)
    r0 = e.bridge(a, b, neff=None)
    assert r0.neff == float(r0.n_post) and r0.logml != r.logml
    same([demc.bridge_chain(chain[:, :, a - 1:b], log_obj[:, a - 1:b], prog, seed=seed).logml], [r0.logml])


def test_bounded_support_program(demc):
    """The isotropic quadratic inside a box: the proposal's draws outside it have a2 = -inf."""
    d, N, G = 2, 64, 200
    c, hbox = np.array([0.2, -0.1]), np.array([0.6, 0.9])
    rng = np.random.default_rng(31)
    w = dict(d=d, K=10, Zinit=np.asfortranarray(c + hbox * rng.uniform(-0.9, 0.9, (128, d))), eps_scale=1e-5 * np.ones(d))
    prog = pt.box_program(c, hbox)
    e = run_engine(demc, prog, w, N, G, 5)
    try:
        e.run(1, G, 2.38)
        r = e.bridge(1, G, neff=None)
        chain, log_obj = e.get_history(1, G)
        box = pt.box_closure(c, hbox)
        ref = br.bridge_f64(chain, log_obj, lambda x: np.array([box(row) for row in x]), seed=demc.bridge_seed(5), fma=br.fma,
                            m=r.mean, L=r.L)
        outside = int(np.isneginf(ref["a2"]).sum())
        assert outside > 0 and r.n_nan == 0 and r.converged
        same(get(e.bridge_proposal(N, G - G // 2, r.mean, r.L))[:, 0, :], ref["a2"])
        ext = br.iterate_ext(ref["a1"], ref["a2"])
        err = abs(r.logml - ext["logml"]) / max(1.0, abs(ext["logml"]))
        exact = sum(math.log(math.sqrt(math.pi) * math.erf(hh)) for hh in hbox)
        print(f"[bridge] box: {outside} of {ref['a2'].size} draws outside, logml {r.logml:.4f} (exact {exact:.4f}, se {r.se_logml:.4f}) err {err:.2e}")
        assert r.iterations == ext["iterations"] and err <= br.LOGML_TOL
    finally:
        e.close()


@pytest.mark.parametrize("layout", ["snooker", "wave"])
def test_other_run_paths(demc, layout):
    """A one-lane handle with snooker generations, and the wave-per-chain layout (the same UNIT_BRIDGE): demcz_bridge works on
    their histories and agrees with the host-array form of the downloaded history bit for bit."""
    d, N, G = 5, 64, 200
    w = demc.workloads.mvnormal_problem(d, N)
    t = w["target"]
    prog = pt.mvn_program(t.mu, t.W, t.c0)
    kw = dict(lanes_per_chain=1) if layout == "snooker" else dict(lanes_per_chain=demc.LAYOUT_PROGRAM_WAVE)
    e = run_engine(demc, prog, w, N, G, 9, **kw)
    try:
        if layout == "snooker":
            e.set_snooker(10)
        e.run(1, G, w["gamma"])
        r = e.bridge(101, G, neff=50.0)
        chain, log_obj = e.get_history(101, G)
        rc = demc.bridge_chain(chain, log_obj, prog, seed=demc.bridge_seed(9), neff=50.0)
        assert r.iterations >= 1 and math.isfinite(r.logml) and math.isfinite(r.se_logml) and r.neff == 50.0
        same([rc.logml, rc.se_logml, rc.ess_f2], [r.logml, r.se_logml, r.ess_f2])
        same(rc.L, r.L)
    finally:
        e.close()


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(demc, e2e):
    e, prog, prob, chain, log_obj = e2e
    ERR_ARG, ERR_STATE = 1, 4
    with pytest.raises(demc.DemczError) as ei:
        e.bridge(10, 12)                                                 # w = 3
    assert ei.value.code == ERR_ARG and "at least 4 generations" in str(ei.value)
    with pytest.raises(demc.DemczError) as ei:
        e.bridge(590, 601, neff=None)
    assert ei.value.code == ERR_ARG and "outside the history window" in str(ei.value)
    # a constant parameter column: the pivot's message names it
    flat = np.array(chain[:, :, :40], order="F")
    flat[:, 1, :] = 0.25
    with pytest.raises(demc.DemczError) as ei:
        demc.bridge_chain(flat, log_obj[:, :40], prog)
    assert ei.value.code == ERR_ARG and "pivot of parameter 1" in str(ei.value)
    # a derived history has no log_obj
    m, L = np.zeros(5), np.asfortranarray(np.eye(5))
    with e.bridge_posterior(401, 600, m, L) as dh:
        out = C.c_void_p()
        lib = _lib.load()
        rc = lib.demcz_bridge_posterior(dh._h, 401, 600, _lib.ptr(m), _lib.ptr(L), C.byref(out))
        assert rc == ERR_STATE and not out.value and b"derived history" in lib.demcz_last_error(dh._h)
        z = [C.c_double() for _ in range(2)]
        rc = lib.demcz_bridge(dh._h, 401, 600, 1, 0.0, 1e-10, 10, C.byref(z[0]), C.byref(z[1]), None, None, None, None, None, None, None,
                              None, None)
        assert rc == ERR_STATE
    # a diagonal of L that is not positive
    Lbad = np.asfortranarray(np.eye(5))
    Lbad[3, 3] = 0.0
    with pytest.raises(demc.DemczError) as ei:
        e.bridge_posterior(401, 600, m, Lbad)
    assert ei.value.code == ERR_ARG and "parameter 3" in str(ei.value)
    # d = 33
    with pytest.raises(demc.DemczError) as ei:
        demc.bridge_chain(np.zeros((4, 33, 8), order="F"), np.zeros((4, 8), order="F"), demc.ProgramTarget(pt.ISO, 33, data=np.zeros(33)))
    assert ei.value.code == ERR_ARG and "1..32" in str(ei.value)
    # a program that does not compile: the log is in last_error
    with pytest.raises(demc.DemczError) as ei:
        demc.bridge_chain(chain[:, :, :40], log_obj[:, :40], demc.ProgramTarget(pt.SYNTAX_ERROR, 5))
    assert ei.value.code == ERR_ARG and "undefined_thing" in str(ei.value)
    # a host-closure handle has no target on the device
    w = demc.workloads.mvnormal_problem(3, 8)
    ec = demc.HipEngine(N=8, d=3, K=10, Mcap=64, Gcap=8, blockindex=[range(3)], eps_scale=w["eps_scale"], seed=1, target=lambda x: 0.0)
    try:
        with pytest.raises(demc.DemczError) as ei:
            ec.bridge(1, 8, neff=None)
        assert ei.value.code == ERR_STATE and "host-closure" in str(ei.value)
    finally:
        ec.close()
