"""GPU: the host-closure kernels in every block structure, form and edge, bit for bit against the oracle.

tests/closure_cases.py holds the worlds: the block structures and one-block dimensions of the block-update and full-update tests
(whose oracle runs they reuse), d = 1 and d = 33, run through demcz_propose / demcz_accept_commit / demcz_end_generation with a
batched closure that is the oracle's own log-density, in the three call modes (copying calls; the pinned buffers; the pinned
buffers with the caller's own arrays), one handle per (world, mode).  Every N x d matrix a demcz_propose returns is compared
with helpers.oracle_sample_logobj's proposal of that (generation, block) -- accepted or not, the columns outside the block
included: they are the current state's bits.  At the end chain, log_obj, X, logp, Z, M, demcz_get_changed per generation and
demcz_get_changed_total (answered from the history: from_ballots == 0) are compared.  The edge worlds run the same comparison;
every refusal of the call protocol is asserted by code and message inside a run that is then carried on and held to the
reference as a whole, so a refused call has consumed no draws and changed no buffer.  No tolerance anywhere (DESIGN.md
section 3)."""
import numpy as np
import pytest

import closure_cases as cc
from helpers import bits_differ, oracle_sample, same_bits

pytestmark = pytest.mark.gpu

KEYS = ("chain", "log_obj", "X", "logp", "Z")
STATE = ("X", "logp", "Z")


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------
def open_engine(demc, case, closure, N=None, chain_id0=0, Gcap=None, Mcap=None, set_state=True):
    w, n = case["problem"], case["N"] if N is None else N
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=n, d=case["d"], K=case["K"], Mcap=M0 + case["N"] * (case["G"] // case["K"] + 1) if Mcap is None else Mcap,
                       Gcap=case["G"] if Gcap is None else Gcap, blockindex=case["blocks"], eps_scale=w["eps_scale"], seed=case["seed"],
                       target=closure, chain_id0=chain_id0)
    if set_state:
        X0 = np.asfortranarray(w["Zinit"][M0 - case["N"]:][chain_id0:chain_id0 + n])
        e.set_state(X0, closure(X0), w["Zinit"])
    return e


def block_step(demc, e, mode, closure, g, ib, gamma, T, want, what):
    """One round trip in `mode`; the proposals that came back are `want`'s bits."""
    if mode == "copies":
        Xp = e.propose(g, ib, gamma)
    elif mode == "pinned":
        bx, bl = e.closure_buffers()
        Xp = e.propose(g, ib, gamma)
        assert Xp is bx
    else:
        bx, _ = e.closure_buffers()
        Xp = np.empty((e.N, e.d), order="F")
        e._chk(e._L.demcz_propose(e._h, g, ib, float(gamma), Xp.ctypes.data_as(demc._lib._dp)))
        assert bits_differ(bx, Xp) is None, f"{what}: the pinned buffer and the caller's array differ"
    why = bits_differ(Xp, want)
    assert why is None, f"{what}: generation {g}, block {ib}: the proposals: {why}"
    if mode == "pinned":
        bl[:] = closure(Xp)
        e.accept_commit(None, T)
    else:
        e.accept_commit(np.array(closure(Xp)), T)


def generations(demc, e, case, closure, loop, mode, g_from, g_to, what=""):
    """Generations g_from..g_to of the case on the handle, every proposal held to the loop's."""
    for g in range(g_from, g_to + 1):
        T = cc.temperature_of(case, g)
        for ib in range(len(case["blocks"])):
            block_step(demc, e, mode, closure, g, ib, case["gamma"], T, loop["xprop"][:, :, g - 1, ib], what)
        e.end_generation(g)


def results(e, g_from=None, g_to=None):
    X, lp, Z, M = e.get_state()
    got = dict(X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M)
    if g_to is not None:
        got["chain"], got["log_obj"] = e.get_history(g_from, g_to)
        got["changed"] = e.get_changed(g_from, g_to)
        got["total"], got["from_ballots"] = e.changed_total(g_from, g_to, with_source=True)
    return got


def held_to(got, ref, what, g_from=1, g_to=None):
    """The run is the reference's, generations g_from..g_to of the history (None: state and archive only)."""
    want = dict(ref)
    if g_to is not None:
        want["chain"], want["log_obj"] = ref["chain"][:, :, g_from - 1:g_to], ref["log_obj"][:, g_from - 1:g_to]
        same_bits(got, want, keys=("chain", "log_obj"), what=what)
        assert np.array_equal(got["changed"], ref["changed"][g_from - 1:g_to]), f"{what}: changed per generation {got['changed']}"
        assert got["total"] == int(ref["changed"][g_from - 1:g_to].sum()) and not got["from_ballots"], f"{what}: changed_total"
    same_bits(got, want, keys=STATE, what=what)
    assert got["M"] == ref["M"], what


def whole_run(demc, oracle, case, mode):
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    what = f"{case['name']}, {mode}"
    e = open_engine(demc, case, closure)
    try:
        if case.get("rng_offset"):
            e.set_rng_offset(case["rng_offset"])
        generations(demc, e, case, closure, loop, mode, 1, case["G"], what=what)
        got = results(e, 1, case["G"])
    finally:
        e.close()
    held_to(got, ref, what, 1, case["G"])
    return got


def refused(demc, code, fragment, call, *args):
    with pytest.raises(demc.DemczError) as err:
        call(*args)
    assert err.value.code == code and fragment in str(err.value), (code, fragment, str(err.value))


# ---- the main worlds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("world", cc.MAIN_WORLDS)
def test_every_block_structure_and_dimension_in_every_call_mode(demc, oracle, world, mode):
    case = cc.main_case(world)
    got = whole_run(demc, oracle, case, mode)
    if world == "left_out":
        X0 = case["problem"]["Zinit"][-case["N"]:]
        for p in (2, 4):
            assert (np.ascontiguousarray(got["chain"][:, p, :]).view(np.uint64) == np.ascontiguousarray(X0[:, p]).view(np.uint64)[:, None]).all(), f"parameter {p} moved"


# ---- populations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
@pytest.mark.parametrize("N", cc.POPULATIONS)
def test_populations_around_the_workgroup_sizes(demc, oracle, N, mode):
    """One, two, three, four and five workgroups of propose_kernel and end_generation_kernel, one and two of accept_commit_kernel,
    the last lane alone; pinned: the flag arrives when the last of them has reported."""
    whole_run(demc, oracle, cc.population_case(N), mode)


# ---- archive boundaries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
@pytest.mark.parametrize("k", [1, 41])
def test_an_append_behind_every_generation_and_none_at_all(demc, oracle, k, mode):
    case = cc.archive_case(k)
    got = whole_run(demc, oracle, case, mode)
    assert got["M"] == case["problem"]["Zinit"].shape[0] + (case["N"] * case["G"] if k == 1 else 0)


@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_the_append_that_would_pass_the_capacity_is_refused(demc, oracle, mode):
    """Mcap is exactly what 40 generations need.  Generation 45's demcz_end_generation is refused before any launch: M, X and the
    archive are what the block-steps of generation 45 left, the history ends at 44."""
    case = cc.capacity_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    M0, N = case["problem"]["Zinit"].shape[0], case["N"]
    e = open_engine(demc, case, closure, Mcap=M0 + N * 8)
    try:
        generations(demc, e, case, closure, loop, mode, 1, 44, what=case["name"])
        for ib in range(len(case["blocks"])):
            block_step(demc, e, mode, closure, 45, ib, case["gamma"], None, loop["xprop"][:, :, 44, ib], case["name"])
        before = results(e, 1, 44)
        refused(demc, demc._lib.ERR_CAPACITY, "Z capacity exceeded", e.end_generation, 45)
        got = results(e, 1, 44)
    finally:
        e.close()
    same_bits(got, before, keys=KEYS, what="the refused call changed a buffer")
    assert got["M"] == before["M"] == M0 + N * 8 == ref["M"] - N
    want = dict(ref, Z=ref["Z"][:M0 + N * 8], M=M0 + N * 8)           # X, logp: generation 45's; the archive: without its rows
    held_to(got, want, case["name"], 1, 44)


# ---- history ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_a_handle_without_history(demc, oracle, mode):
    """Gcap = 0: end_generation_kernel is handed null history pointers.  demcz_get_history is refused, and so is
    demcz_get_changed_total: a closure handle has no ballots, its total is counted from the history (ERR_STATE, "keeps no history")."""
    case = cc.no_history_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    e = open_engine(demc, case, closure, Gcap=0)
    try:
        generations(demc, e, case, closure, loop, mode, 1, case["G"], what=case["name"])
        refused(demc, demc._lib.ERR_STATE, "keeps no history", e.get_history, 1, case["G"])
        refused(demc, demc._lib.ERR_STATE, "keeps no history", e.changed_total, 1, case["G"])
        got = results(e)
    finally:
        e.close()
    held_to(got, ref, case["name"])


@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_a_moved_history_origin(demc, oracle, mode):
    """Gcap = 20.  demcz_set_history_origin(20) behind generation 20: generations 21..40 land in slots 0..19; generation 41 is
    outside the window and its demcz_end_generation is refused."""
    case = cc.origin_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    e = open_engine(demc, case, closure, Gcap=cc.ORIGIN)
    try:
        generations(demc, e, case, closure, loop, mode, 1, cc.ORIGIN, what=case["name"])
        first = results(e, 1, cc.ORIGIN)
        e.set_history_origin(cc.ORIGIN)
        generations(demc, e, case, closure, loop, mode, cc.ORIGIN + 1, 2 * cc.ORIGIN, what=case["name"])
        refused(demc, demc._lib.ERR_INVALID_ARGUMENT, "outside the history window", e.get_history, cc.ORIGIN, 2 * cc.ORIGIN)
        second = results(e, cc.ORIGIN + 1, 2 * cc.ORIGIN)
        g = 2 * cc.ORIGIN + 1
        for ib in range(len(case["blocks"])):
            block_step(demc, e, mode, closure, g, ib, case["gamma"], cc.temperature_of(case, g), loop["xprop"][:, :, g - 1, ib], case["name"])
        refused(demc, demc._lib.ERR_CAPACITY, "outside the history window", e.end_generation, g)
        last = results(e, cc.ORIGIN + 1, 2 * cc.ORIGIN)
    finally:
        e.close()
    for k in ("chain", "log_obj"):
        assert bits_differ(first[k], ref[k][..., :cc.ORIGIN]) is None, k
    assert np.array_equal(first["changed"], ref["changed"][:cc.ORIGIN])
    same_bits(last, second, keys=("chain", "log_obj"), what="the refused call changed the history")
    held_to(last, ref, case["name"], cc.ORIGIN + 1, 2 * cc.ORIGIN)        # X, logp, Z: behind generation 41's block-steps


# ---- the draw stream ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_a_stream_offset(demc, oracle, mode):
    """demcz_set_rng_offset(7): the Philox block of generation g is (g + 7 - 1) S + ..."""
    case = cc.rng_offset_case()
    assert case["rng_offset"] == 7
    whole_run(demc, oracle, case, mode)


def test_prevrun_carried_into_a_closure_run_with_other_blocks(demc, oracle):
    """The closure twin of test_gpu_parity's test_prevrun_carried_into_a_run_with_other_blocks_equals_oracle: the second run starts
    from the CARRIED log-densities (made under one block) and its streams start behind everything the first run drew."""
    from demc_jl_amd.sampler import blocks_per_generation
    p = cc.PREVRUN
    d, N, K, G1, G2, seed, gamma, b2 = p["d"], p["N"], p["K"], p["G1"], p["G2"], p["seed"], p["gamma"], p["second"]
    w = demc.workloads.mvnormal_problem(d, N)
    closures = []
    for blocks in (None, b2):
        prob = oracle.Problem(N, d, K, 10, w["eps_scale"], 0, blocks=blocks, target=w["target"].spec())
        f = (lambda pr: lambda X: oracle.logp(pr, np.asarray(X)))(prob)
        f.batched = True
        closures.append(f)
    S1, S2 = blocks_per_generation([range(d)]), blocks_per_generation(b2)
    assert S1 != S2
    mc1, Z1 = demc.demcz_sample(closures[0], w["Zinit"], N, K, G1, 1, [range(d)], w["eps_scale"], gamma, verbose=False, seed=seed)
    mc2, Z2 = demc.demcz_sample(closures[1], Z1, N, K, G2, len(b2), b2, w["eps_scale"], gamma, verbose=False, seed=seed, prevrun=mc1)
    r1 = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G1, None, w["eps_scale"], gamma, seed)
    same_bits(dict(chain=mc1.chain, log_obj=mc1.log_obj, X=mc1.Xcurrent, logp=mc1.log_objcurrent, Z=Z1), r1, what="the first run")
    r2 = oracle_sample(oracle, w["target"], r1["Z"], N, K, G2, b2, w["eps_scale"], gamma, seed, X0=r1["X"], lp0=r1["logp"],
                       rng_offset=-(-G1 * S1 // S2))
    same_bits(dict(chain=mc2.chain[:, :, G1:], log_obj=mc2.log_obj[:, G1:], X=mc2.Xcurrent, logp=mc2.log_objcurrent, Z=Z2), r2, what="the resumed run")
    assert bits_differ(oracle.logp(r2["prob"], r1["X"]), r1["logp"]) is not None, "the carried values must differ from the run's own evaluation"
    assert (r2["changed"] > 0).all()


# ---- shards --------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_appended_from_the_host(demc, oracle):
    """Two closure handles of 48 chains (chain_id0 = 0 and 48), demcz_set_external_append; at every K boundary the host appends the
    96 current rows in chain order to both (demcz_append_rows).  Shard 0 in copying mode, shard 1 on the pinned buffers."""
    case = cc.plain_edge_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    half, G = case["N"] // 2, case["G"]
    shards = [open_engine(demc, case, closure, N=half, chain_id0=c0) for c0 in (0, half)]
    try:
        for e in shards:
            e.set_external_append(True)
        for g in range(1, G + 1):
            T = cc.temperature_of(case, g)
            for ib in range(len(case["blocks"])):
                for s, (e, mode) in enumerate(zip(shards, ("copies", "pinned"))):
                    block_step(demc, e, mode, closure, g, ib, case["gamma"], T, loop["xprop"][s * half:(s + 1) * half, :, g - 1, ib], f"shard {s}")
            for e in shards:
                e.end_generation(g)
            if g % case["K"] == 0:
                rows = np.concatenate([e.get_state(with_Z=False)[0] for e in shards], axis=0)
                for e in shards:
                    e.append_rows(rows)
        got = [results(e, 1, G) for e in shards]
    finally:
        for e in shards:
            e.close()
    both = {k: np.concatenate([g[k] for g in got], axis=0) for k in ("chain", "log_obj", "X", "logp")}
    same_bits(both, ref, keys=("chain", "log_obj", "X", "logp"), what="the shards side by side")
    for s, g in enumerate(got):
        assert g["M"] == ref["M"] and bits_differ(g["Z"], ref["Z"]) is None, f"shard {s}: the archive"
    assert np.array_equal(got[0]["changed"] + got[1]["changed"], ref["changed"])


def test_a_one_rank_communicator(demc, oracle):
    """demcz_comm_init(…, 1, 0) on a closure handle: demcz_end_generation appends through append_after_window (the all-gather of
    the one rank).  The bits of the plain handle; no peers."""
    case = cc.plain_edge_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    e = open_engine(demc, case, closure, set_state=False)
    try:
        e.comm_init(e.comm_unique_id(), 1, 0)
        X0 = np.asfortranarray(case["problem"]["Zinit"][-case["N"]:])
        e.set_state(X0, closure(X0), case["problem"]["Zinit"])
        generations(demc, e, case, closure, loop, "pinned", 1, case["G"], what="one-rank communicator")
        got = results(e, 1, case["G"])
        status = e.peer_status()
    finally:
        e.close()
    held_to(got, ref, "one-rank communicator", 1, case["G"])
    assert status == (0, 0)


# ---- temperatures and closure values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
@pytest.mark.parametrize("which", [0, 1], ids=["d6_blocks", "d64_one_block"])
def test_zero_tiny_and_huge_temperatures(demc, oracle, which, mode):
    case = cc.zero_temperature_cases()[which]
    assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist())
    whole_run(demc, oracle, case, mode)


@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_a_closure_that_returns_infinities_and_nan(demc, oracle, mode):
    """The box closure: -inf outside, NaN behind one face, +inf in one cell.  The reference decides in IEEE float64
    (helpers.oracle_sample_logobj): a NaN difference rejects, a chain at +inf stays."""
    case = cc.box_case()
    got = whole_run(demc, oracle, case, mode)
    assert np.isposinf(got["logp"]).any() and not np.isnan(got["log_obj"]).any() and not np.isneginf(got["log_obj"]).any()


# ---- switching modes ---------------------------------------------------------------------------------------------------------------------------
def test_switching_to_the_pinned_buffers_inside_a_run(demc, oracle):
    case = cc.switch_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    e = open_engine(demc, case, closure)
    try:
        generations(demc, e, case, closure, loop, "copies", 1, cc.SWITCH_AT, what="copies")
        e.closure_buffers()
        generations(demc, e, case, closure, loop, "pinned", cc.SWITCH_AT + 1, case["G"], what="pinned behind copies")
        got = results(e, 1, case["G"])
    finally:
        e.close()
    held_to(got, ref, case["name"], 1, case["G"])


# ---- the sampler surface -----------------------------------------------------------------------------------------------------------------------
def _surface(demc, oracle):
    s = cc.SURFACE
    w = demc.workloads.mvnormal_problem(s["d"], s["N"])
    prob = oracle.Problem(s["N"], s["d"], s["K"], 10, w["eps_scale"], 0, blocks=s["blocks"], target=w["target"].spec())
    args = (w["Zinit"], s["N"], s["K"], s["G"], len(s["blocks"]), s["blocks"], w["eps_scale"], s["gamma"])
    return s, w, prob, args


def test_a_per_row_closure_and_the_same_closure_batched(demc, oracle):
    s, w, prob, args = _surface(demc, oracle)
    T = cc.bc.temperatures(s["G"])
    shapes = []
    per_row = lambda x: float(oracle.logp(prob, np.asarray(x)[None, :])[0])      # noqa: E731

    def batched(X):
        X = np.asarray(X)
        shapes.append(X.shape)
        return oracle.logp(prob, X)
    batched.batched = True
    kw = dict(verbose=False, seed=s["seed"], adaptγ={"adapt": False}, temperaturefun=lambda ig, Ng, T0, TN: float(T[ig - 1]))
    a, Za = demc.demcz_anneal(per_row, *args, **kw)
    b, Zb = demc.demcz_anneal(batched, *args, **kw)
    assert shapes.count((s["N"], s["d"])) >= s["G"] * len(s["blocks"]) + 1          # (+ the starting values)
    same_bits(dict(chain=a.chain, log_obj=a.log_obj, Z=Za), dict(chain=b.chain, log_obj=b.log_obj, Z=Zb), keys=("chain", "log_obj", "Z"), what="per row against batched")
    ref = oracle_sample(oracle, w["target"], w["Zinit"], s["N"], s["K"], s["G"], s["blocks"], w["eps_scale"], s["gamma"], s["seed"], temperature=T)
    same_bits(dict(chain=b.chain, log_obj=b.log_obj, Z=Zb), ref, keys=("chain", "log_obj", "Z"), what="batched against the oracle")


def test_gamma_adapted_from_the_changed_total_of_a_closure_run(demc, oracle):
    """demcz_anneal adapts gamma every ten generations from demcz_get_changed_total -- the ballots of a device target, the history
    of a closure handle: the same run, at d = 6 in blocks."""
    s, w, prob, args = _surface(demc, oracle)
    closure = lambda X: oracle.logp(prob, np.asarray(X))      # noqa: E731
    closure.batched = True
    kw = dict(verbose=False, T0=2, TN=1e-2, seed=s["seed"], adaptγ={"adapt_every": 10})
    a, Za = demc.demcz_anneal(closure, *args, **kw)
    b, Zb = demc.demcz_anneal(w["target"], *args, **kw)
    same_bits(dict(chain=a.chain, log_obj=a.log_obj, Z=Za), dict(chain=b.chain, log_obj=b.log_obj, Z=Zb), keys=("chain", "log_obj", "Z"), what="closure against device target")
    c, _ = demc.demcz_anneal(w["target"], *args, **dict(kw, adaptγ={"adapt": False}))
    assert bits_differ(c.chain, b.chain) is not None, "the adaptation must change the run"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cc.EDGE_MODES)
def test_the_refusals_of_the_call_protocol_leave_the_run_alone(demc, oracle, mode):
    case = cc.plain_edge_case()
    closure, ref, loop = cc.batched_closure(oracle, case), cc.reference(oracle, case), cc.proposal_loop(oracle, case)
    ERR_ARG, ERR_STATE = demc._lib.ERR_INVALID_ARGUMENT, demc._lib.ERR_STATE
    NB, gamma, N, d = len(case["blocks"]), case["gamma"], case["N"], case["d"]
    lp = np.zeros(N)
    e = open_engine(demc, case, closure, set_state=False)
    try:
        refused(demc, ERR_STATE, "call demcz_set_state first", e.propose, 1, 0, gamma)
        X0 = np.asfortranarray(case["problem"]["Zinit"][-N:])
        e.set_state(X0, closure(X0), case["problem"]["Zinit"])
        refused(demc, ERR_STATE, "no pending proposal", e.accept_commit, lp)
        refused(demc, ERR_STATE, "no open generation", e.end_generation, 1)
        refused(demc, ERR_ARG, "bad generation or block", e.propose, 1, NB, gamma)
        refused(demc, ERR_ARG, "bad generation or block", e.propose, 0, 0, gamma)
        with pytest.raises(ValueError, match="closure_buffers"):
            e.accept_commit(None)
        # without the pinned buffers a null Xprop is refused -- and has opened no generation
        assert e._L.demcz_propose(e._h, 1, 0, float(gamma), None) == ERR_ARG and b"Xprop is required" in e._L.demcz_last_error(e._h)
        refused(demc, ERR_STATE, "no open generation", e.end_generation, 1)
        if mode == "pinned":
            e.closure_buffers()
        generations(demc, e, case, closure, loop, mode, 1, 7, what="before the refusals")
        # inside generation 8: a proposal pending
        g, T = 8, cc.temperature_of(case, 8)
        Xp = e.propose(g, 0, gamma)
        assert bits_differ(Xp, loop["xprop"][:, :, g - 1, 0]) is None
        values = np.array(closure(Xp))
        refused(demc, ERR_STATE, "previous proposal not committed", e.propose, g, 1, gamma)
        refused(demc, ERR_STATE, "uncommitted proposal", e.end_generation, g)
        if mode == "pinned":
            e.closure_buffers()[1][:] = values
            e.accept_commit(None, T)
        else:
            e.accept_commit(values, T)
        refused(demc, ERR_STATE, "no pending proposal", e.accept_commit, lp, T)
        refused(demc, ERR_ARG, "bad generation or block", e.propose, g, NB, gamma)
        for ib in range(1, NB):
            block_step(demc, e, mode, closure, g, ib, gamma, T, loop["xprop"][:, :, g - 1, ib], "behind the refusals")
        e.end_generation(g)
        refused(demc, ERR_STATE, "no open generation", e.end_generation, g)
        # a handle of the wrong kind
        refused(demc, ERR_STATE, "host-callback target uses demcz_propose", e.run, g + 1, g + 2, gamma)
        refused(demc, ERR_STATE, "no snooker generations", e.set_snooker, 2)
        refused(demc, ERR_STATE, "host-closure handle has no target on the device", e.bridge, 1, g, None, None)
        # an append lag: accepted by demcz_set_append_lag, refused by demcz_end_generation
        e.set_append_lag(1)
        for ib in range(NB):
            block_step(demc, e, mode, closure, g + 1, ib, gamma, cc.temperature_of(case, g + 1), loop["xprop"][:, :, g, ib], "with a lag set")
        refused(demc, ERR_STATE, "append lag 0", e.end_generation, g + 1)
        e.set_append_lag(0)
        e.end_generation(g + 1)
        generations(demc, e, case, closure, loop, mode, g + 2, case["G"], what="behind the refusals")
        got = results(e, 1, case["G"])
    finally:
        e.close()
    held_to(got, ref, f"{case['name']}, {mode}: the run around the refusals", 1, case["G"])


def test_the_closure_calls_refuse_a_device_target_handle(demc):
    w = demc.workloads.mvnormal_problem(5, 8)
    e = demc.HipEngine(N=8, d=5, K=5, Mcap=w["Zinit"].shape[0] + 16, Gcap=5, blockindex=[range(5)], eps_scale=w["eps_scale"], seed=1, target=w["target"])
    try:
        e.set_state(w["Zinit"][-8:], None, w["Zinit"])
        ERR_STATE = demc._lib.ERR_STATE
        refused(demc, ERR_STATE, "not created with DEMCZ_TARGET_HOST_CALLBACK", e.propose, 1, 0, 0.5)
        refused(demc, ERR_STATE, "not created with DEMCZ_TARGET_HOST_CALLBACK", e.closure_buffers)
        refused(demc, ERR_STATE, "host-callback handles only", e.end_generation, 1)
        e.run(1, 5, 0.5)                                   # (and the handle still runs)
    finally:
        e.close()
