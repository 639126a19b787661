"""Non-finite log-densities and states through every kernel layout, against the oracle, bit for bit.

DESIGN.md section 3 states how such values behave -- accept is log u < lp' - lp, strict, so a NaN difference rejects; `changed`
is (lp_after - lp_before) != 0, so a NaN difference counts -- and the kernels hold code for them that nothing else reaches: the
wave-per-chain kernels select among 31 speculative candidates with ballots, the block kernel keeps partial sums across rejected
proposals, the replicated consumer filters unpublished rows by the high word of a NaN, the matrix form of the wave kernel has a
path for non-finite increments only.  The comparison is helpers.same_bits (it sees a lost sign of zero; a NaN's payload is
unspecified), the inputs are nonfinite_cases.py's, whose oracle runs test_nonfinite_reference.py has checked on the CPU:
  1. every built-in row of test_gpu_kernel_choice.py's table on a poisoned population, with what the handle says about itself
     held to the fixture recorded on finite data (non-finite data must not move a run to another kernel or cost a redo);
  2. three worlds whose arithmetic is subnormal, on the rows whose DPP / matrix-instruction chains they reach;
  3. the matrix form of window_kernel_pw on a poisoned population: the documented redo, the oracle's result;
  4. demcz_run_checked with R-hat vectors that hold NaN;
  5. program targets that return -inf, NaN and +inf or loop a data-dependent number of times, on the one-lane layout, the
     wave-per-chain layout and the host-closure path, against the oracle's loop around the program's Python twin."""
import json

import numpy as np
import pytest

import demc_jl_amd as demc
import nonfinite_cases as nf
from demc_jl_amd import _lib
from helpers import bits_differ, poisoned_population, same_bits
from test_gpu_kernel_choice import CASES, FIXTURE
from test_gpu_program_wave import _wave_name

pytestmark = pytest.mark.gpu

WAVE, PROGRAM_WAVE = _lib.LAYOUT_SPLIT_WAVE, _lib.LAYOUT_PROGRAM_WAVE


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def _run(r, calls, lanes=None, target=None, observe=None):
    """One handle through `calls` [(g_from, g_to, temperatures or None)]; the initial log-densities are the device's.  `observe`
    receives what the handle says about itself after every call."""
    Zinit, N, d, K, G = np.asfortranarray(r["Zinit"]), r["N"], r["d"], r["K"], r["G"]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Zinit.shape[0] + N * (G // K + 1), Gcap=G, blockindex=r.get("blocks") or [range(d)],
                       eps_scale=r["eps"], seed=r["seed"], target=r["target"] if target is None else target,
                       lanes_per_chain=r["lanes"] if lanes is None else lanes)
    try:
        e.set_state(Zinit[-N:], None, Zinit)
        for a, b, T in calls:
            e.run(a, b, r["gamma"], temperature=T)
            if observe is not None:
                e.synchronize()
                info = e.info()
                observe.append(dict(kernel_name=e.kernel_name(), live_status=list(e.live_status()),
                                    lanes_per_chain=info["lanes_per_chain"], window_launches=info["window_launches"]))
        e.synchronize()
        chain, lobj = e.get_history(1, G)
        X, lp, Z, M = e.get_state()
        total, from_ballots = e.changed_total(1, G, with_source=True)
        out = dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z), M=M, changed=e.get_changed(1, G),
                   changed_total=total, from_ballots=from_ballots, name=e.kernel_name(), live=e.live_status(), info=e.info())
    finally:
        e.close()
    return out


def _same_run(got, ref, what):
    same_bits(got, ref, what=what)
    assert got["M"] == ref["M"], what
    assert np.array_equal(got["changed"], ref["changed"]), f"{what}: changed per generation {got['changed']}, oracle {ref['changed']}"
    assert got["changed_total"] == int(ref["changed"].sum()), \
        f"{what}: changed_total {got['changed_total']} (from the ballots: {got['from_ballots']}), oracle {int(ref['changed'].sum())}"


def _calls(r):
    """The calls of a row (two plain, one tempered) or of a world (the same cuts, all plain or all tempered)."""
    p = nf.pieces(r["K"])
    if "T" in r:
        return [p[0] + (None,), p[1] + (None,), p[2] + (r["T"],)]
    T = r["temperature"]
    return [(a, b, None if T is None else T[a - 1:b]) for a, b in p]


# ---- 1. every built-in row of the kernel-choice table -------------------------------------------------------------------------
@pytest.mark.parametrize("case", nf.BUILTIN_ROWS)
def test_poisoned_population_on_every_kernel_equals_oracle(oracle, recorded, case):
    r = nf.row_inputs(case)
    seen = []
    got = _run(r, _calls(r), observe=seen)
    ref = nf.reference(oracle, r)
    print(f"{case}: changed_total from the {'ballots' if got['from_ballots'] else 'history'}; {[s['kernel_name'] for s in seen]}")
    _same_run(got, ref, case)
    for i, (s, want) in enumerate(zip(seen, recorded[case]["pieces"])):
        for field in ("kernel_name", "lanes_per_chain", "window_launches", "live_status"):
            assert s[field] == want[field], f"{case}, call {i}: {field}: {s[field]!r}, recorded on finite data {want[field]!r}"


# ---- 2. subnormal worlds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,case,tempered", nf.WORLD_CASES)
def test_subnormal_worlds_equal_oracle(oracle, recorded, world, case, tempered):
    r = nf.world_inputs(world, case, tempered)
    seen = []
    got = _run(r, _calls(r), observe=seen)
    ref = nf.reference(oracle, r)
    _same_run(got, ref, f"{world} {case}")
    # the row's kernels: the fixture's first two calls are plain and its third tempered, with the same cuts
    for i in ([2] if tempered else [0, 1]):
        assert seen[i]["kernel_name"] == recorded[case]["pieces"][i]["kernel_name"], (i, seen)
    assert seen[-1]["live_status"] == recorded[case]["pieces"][-1]["live_status"], seen
    if world == "mvn":
        assert not got["changed"].any() and nf.subnormal_share(got["chain"]) >= 0.9
    else:
        assert nf.subnormal_share(got["log_obj"]) >= 0.9


# ---- 3. the matrix form's redo ----------------------------------------------------------------------------------------------------
def test_matrix_form_redoes_a_pass_with_a_nonfinite_increment(oracle, monkeypatch):
    """window_kernel_pw<MVNORMAL, 20, LIVE, ., MF = true> forms its candidates as x + Delta T with 0 * delta where the serial order
    adds -0.0: a non-finite increment would poison the candidates that do not take it, so such a pass flags the launch and the
    library redoes it with the scalar kernels (demcz_kernels_pw.h).  The redo is expected; the result is the oracle's."""
    monkeypatch.setenv("DEMCZ_PW_MFMA", "1")
    d, N, K = 20, 100, 5
    w = demc.workloads.mvnormal_problem(d, N)
    eps = np.array(w["eps_scale"])
    eps[0] = 1e-320
    r = dict(target=w["target"], gamma=w["gamma"], d=d, N=N, K=K, G=6 * K + 3, lanes=WAVE, blocks=None, eps=eps,
             Zinit=poisoned_population(d, N, nf.POPULATION_SEED), seed=nf.RUN_SEED,
             T=np.array([demc.tempbaseline(g, 2 * K, 3, 1e-3) for g in range(1, 2 * K + 1)]))
    seen = []
    got = _run(r, _calls(r), observe=seen)
    ref = nf.reference(oracle, r)
    print([(s["kernel_name"], s["live_status"]) for s in seen])
    _same_run(got, ref, "matrix form")
    assert got["live"][1] >= 1, got["live"]


# ---- 4. demcz_run_checked -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poisoned", [True, False])
def test_run_checked_with_nonfinite_rhat_is_the_driver_loop(oracle, poisoned):
    """wave_mvn_d5's shape through demcz_run_checked, a check every 2K generations, threshold 1.1, against the same host logic
    over the oracle (sampler.py's loop: stop when max(Rhat) < threshold; a NaN maximum never is).  On the poisoned population the
    R-hat vectors hold NaN -- at the oracle's positions; on the clean one they are finite.  Finite values within the project's
    stated 1e-9 relative."""
    from oracle_engine import OracleEngine
    kind, d, N, K, lanes, blocks, nobs = CASES["wave_mvn_d5"]
    w = demc.workloads.mvnormal_problem(d, N)
    Zinit = poisoned_population(d, N, nf.POPULATION_SEED) if poisoned else np.asfortranarray(w["Zinit"])
    every, thr, G = 2 * K, 1.1, 12 * K
    kw = dict(N=N, d=d, K=K, Mcap=Zinit.shape[0] + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"],
              seed=nf.RUN_SEED, target=w["target"])
    o = OracleEngine(**kw)
    o.set_state(Zinit[-N:], None, Zinit)
    g_ref, trace, last_ref = G, [], None
    for g in range(every, G + 1, every):
        o.run(g - every + 1, g, w["gamma"])
        last_ref = o.rhat(g - every + 1, g)
        trace.append(float(np.max(last_ref)))
        if trace[-1] < thr:
            g_ref = g
            break
    e = demc.HipEngine(lanes_per_chain=lanes, **kw)
    try:
        e.set_state(Zinit[-N:], None, Zinit)
        g_stop, mx, last = e.run_checked(1, G, w["gamma"], every, thr)
        chain, lobj = e.get_history(1, g_stop)
        live = e.live_status()
    finally:
        e.close()
    print(f"poisoned={poisoned}: g_stop {g_stop} (oracle {g_ref}), last R-hat {last}, oracle {last_ref}")
    assert g_stop == g_ref and len(mx) == len(trace)
    assert bits_differ(chain, o.chain[:, :, :g_stop]) is None and bits_differ(lobj, o.log_obj[:, :g_stop]) is None
    for got, want in ((last, last_ref), (mx, np.array(trace))):
        assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
        f = ~np.isnan(want)
        assert np.array_equal(np.isinf(got[f]), np.isinf(want[f])) and np.array_equal(np.sign(got[f]), np.sign(want[f])), (got, want)
        f &= np.isfinite(want)
        assert np.all(np.abs(got[f] - want[f]) <= 1e-9 * np.abs(want[f])), (got, want)
    assert np.isnan(last_ref).any() if poisoned else np.isfinite(last_ref).all()
    assert live == (True, 0), live


# ---- 5. program targets -------------------------------------------------------------------------------------------------------------
def _host_closure_run(r, calls):
    """The host-closure path: the Python twin as the target, one demcz_propose / demcz_accept_commit round trip per generation."""
    Zinit, N, d, K, G = np.asfortranarray(r["Zinit"]), r["N"], r["d"], r["K"], r["G"]
    closure = lambda X: np.array([r["twin"]([float(v) for v in x]) for x in np.asarray(X)])
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Zinit.shape[0] + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=r["eps"],
                       seed=r["seed"], target=closure)
    try:
        e.set_state(Zinit[-N:], closure(Zinit[-N:]), Zinit)
        T = r["temperature"]
        for g in range(1, G + 1):
            e.accept_commit(closure(e.propose(g, 0, r["gamma"])), None if T is None else float(T[g - 1]))
            e.end_generation(g)
        chain, lobj = e.get_history(1, G)
        X, lp, Z, M = e.get_state()
        out = dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z), M=M, changed=e.get_changed(1, G),
                   changed_total=e.changed_total(1, G), from_ballots=False)
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name,d,N,tempered", nf.PROGRAM_GRID)
def test_program_targets_off_the_finite_line_equal_the_python_twin(oracle, name, d, N, tempered):
    """d = 2, 5: window_kernel_ps; d = 7, 20: window_kernel_pw.  K = 5, 45 generations in calls that start and end off the
    boundaries.  The conditions on the reference make sure the case holds what it is for (see nonfinite_cases.program_inputs)."""
    r = nf.program_inputs(name, d, N, tempered)
    ref = nf.program_reference(oracle, r)
    facts = nf.program_reference_facts(r, ref)
    print(name, d, N, tempered, facts)
    assert 2 * facts["moved"] >= N
    if name in ("box", "sqrtdom"):
        assert 0.15 * N <= facts["outside_at_start"] <= 0.4 * N and facts["finite_chain_rejected_outside"] >= 1
    if name in ("box", "box_poisoned"):
        assert facts["entered"] >= 1                        # -inf outside: the first candidate inside is accepted
    if name == "sqrtdom":
        assert facts["entered"] == 0                        # NaN outside: every difference is NaN and rejects -- such a chain stays
    if name == "pole":
        assert facts["captured"] >= 1 and 2 * facts["captured"] <= N and facts["captured"] > facts["captured_at_start"]
    T = r["temperature"]
    calls = [(a, b, None if T is None else T[a - 1:b]) for a, b in nf.PROGRAM_CALLS]
    lane = _run(r, calls, lanes=1)
    assert "(program)" in lane["name"] and "window_kernel<4," in lane["name"], lane["name"]
    _same_run(lane, ref, f"{name} d={d} N={N}, one lane per chain")
    wave = _run(r, calls, lanes=PROGRAM_WAVE)
    _wave_name(wave["name"], d)
    _same_run(wave, ref, f"{name} d={d} N={N}, wave per chain")
    assert wave["live"] == (True, 0), wave["live"]
    host = _host_closure_run(r, calls)
    _same_run(host, ref, f"{name} d={d} N={N}, host closure")
