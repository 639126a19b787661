"""The counting kernel of the quantiles' radix select (K9, demcz_kernels_sel.h), demcz_quantiles around it, the arg-max kernels of
demcz_best and their Python faces against the reference of quantile_cases.py: chain blocks that are not full, many time chunks,
one chain, one draw, parameters 1e6 standard deviations from zero (every draw of a wave in one bin), +-0.0, +-inf, subnormals,
runs of duplicates, NaNs of either sign; windows inside a handle's history; host shards and the communicator routes.  lower and
upper are compared as uint64, q with equal_nan: no tolerance anywhere.  test_quantile_reference.py shows without a GPU that the
worlds reach the cases they are for."""
import numpy as np
import pytest

import quantile_cases as Q
import stats_cases as S

pytestmark = pytest.mark.gpu

PROBS = Q.PROBS


def hold(got, ref, what):
    for name, a, b in zip(("q", "lower", "upper"), got, ref):
        bad = np.argwhere(~((Q.bits(a) == Q.bits(b)) | (np.isnan(a) & np.isnan(b) & (name == "q"))))
        if bad.size:
            p, j = bad[0]
            print(f"[quantiles] {what}: {name} differs at {len(bad)} places, first (parameter {p}, prob {j}): {a[p, j]!r} vs {b[p, j]!r}")
    assert Q.same(got, ref), what


# ---- the array entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", Q.ARRAY_WORLDS, ids=Q.ids)
def test_quantile_chain_on_the_worlds(demc, w):
    chain = S.world(*w)
    got = demc.quantile_chain(chain, PROBS, with_order_stats=True)
    hold(got, Q.world_reference(w), Q.ids(w))
    assert np.array_equal(demc.quantile_chain(chain, PROBS), got.q)


def test_one_draw_and_identical_draws(demc):
    hold(demc.quantile_chain(Q.one_draw(), PROBS, with_order_stats=True), Q.reference(Q.one_draw()), "1x1x1")
    same = S.all_identical()
    got = demc.quantile_chain(same, PROBS, with_order_stats=True)
    hold(got, Q.reference(same), "identical")
    assert (got.q == 1000000.25).all()


def test_low_byte_and_repeated_worlds(demc):
    for name, chain in (("low byte", Q.low_byte_world()), ("repeated", Q.repeated_world())):
        hold(demc.quantile_chain(chain, PROBS, with_order_stats=True), Q.reference(chain), name)


# ---- special values ------------------------------------------------------------------------------------------------------------------
def test_signed_zeros_infinities_subnormals_and_duplicates(demc):
    hold(demc.quantile_chain(Q.specials(), PROBS, with_order_stats=True), Q.reference(Q.specials()), "specials")


@pytest.mark.parametrize("negative", [False, True], ids=["+nan", "-nan"])
def test_a_nan_spoils_its_own_parameter_only(demc, negative):
    clean = demc.quantile_chain(Q.specials(), PROBS, with_order_stats=True)
    got = demc.quantile_chain(Q.with_nan(negative), PROBS, with_order_stats=True)
    hold(got, Q.reference(Q.with_nan(negative)), "one NaN")
    for a, b in zip(got, clean):
        assert np.isnan(a[1]).all() and np.array_equal(Q.bits(a[[0, 2]]), Q.bits(b[[0, 2]]))


# ---- limits --------------------------------------------------------------------------------------------------------------------------
def test_probability_count_and_range(demc):
    chain = S.world(64, 3, 260)
    one = demc.quantile_chain(chain, [0.5], with_order_stats=True)
    hold(one, Q.reference(chain, [0.5]), "nq = 1")
    sixteen = tuple(np.linspace(0.0, 1.0, 16))
    hold(demc.quantile_chain(chain, sixteen, with_order_stats=True), Q.reference(chain, sixteen), "nq = 16")
    for bad in (tuple(np.linspace(0.0, 1.0, 17)), (0.5, -0.1), (np.nan,), ()):
        with pytest.raises(demc.DemczError) as ei:
            demc.quantile_chain(chain, bad)
        assert ei.value.code == 1, bad
    mixed = (0.975, 0.5, 0.5, 0.0, 1.0, 0.025, 0.5, 1.0 / 3.0)
    got = demc.quantile_chain(chain, mixed, with_order_stats=True)
    hold(got, Q.reference(chain, mixed), "repeated and unsorted")
    for j, q in enumerate(mixed):
        single = demc.quantile_chain(chain, [q], with_order_stats=True)
        for a, b in zip(got, single):
            assert np.array_equal(Q.bits(a[:, j]), Q.bits(b[:, 0])), q


# ---- the counting pass ---------------------------------------------------------------------------------------------------------------
def _engine(demc, w, N, d, G, Gcap, seed=21, K=10, comm=False):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=Gcap, blockindex=[range(d)], eps_scale=w["eps_scale"],
                       seed=seed, target=w["target"])
    if comm:
        e.comm_init(e.comm_unique_id(), 1, 0)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


@pytest.fixture(scope="module")
def history(demc):
    """One engine with 130 generations of a d = 20, N = 300 run, shared by the tests that only read it."""
    d, N, G = 20, 300, 130
    e = _engine(demc, demc.workloads.mvnormal_problem(d, N), N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    yield e
    e.close()


def test_select_counts(demc, history):
    e = history
    d, N = e.d, e.N
    for a, b in [(1, 130), (37, 101), (77, 77)]:
        ch = e.get_history(a, b)[0]
        zero = np.zeros((d, 1), dtype=np.uint64)
        counts, nan = e.select_counts(a, b, 56, zero)
        want, wnan = Q.count_pass(ch, 56, zero)
        assert np.array_equal(counts, want) and (counts.sum(axis=(1, 2)) == N * (b - a + 1)).all() and np.array_equal(nan, wnan) and not nan.any()
        # at shift 56 every draw matches every prefix, whatever its value
        three, _ = e.select_counts(a, b, 56, np.array([[5, 0, 9]] * d, dtype=np.uint64))
        assert np.array_equal(three, np.repeat(want, 3, axis=1))
        # a middle byte under two prefixes: the two most frequent top-three-byte prefixes of every parameter (and 3, 5, 32 columns
        # with padding that matches nothing)
        shift = 32
        top = np.empty((d, 2), dtype=np.uint64)
        for p in range(d):
            v, c = np.unique(Q.keys(Q.draws(ch, p)) >> np.uint64(shift + 8), return_counts=True)
            top[p] = v[np.argsort(-c, kind="stable")[:2]] if v.size > 1 else [v[0], ~np.uint64(0)]
        for npre in (2, 3, 5, 32):
            pre = np.full((d, npre), ~np.uint64(0), dtype=np.uint64)
            pre[:, :2] = top
            counts, nan = e.select_counts(a, b, shift, pre)
            want, _ = Q.count_pass(ch, shift, pre)
            assert np.array_equal(counts, want) and counts[:, :2].sum() > 0 and not counts[:, 2:].any(), (a, b, npre)
    for shift, npre in [(57, 1), (-8, 1), (4, 1), (64, 1), (8, 33), (8, 0)]:
        with pytest.raises(demc.DemczError) as ei:
            e.select_counts(1, 130, shift, np.zeros((d, npre), dtype=np.uint64))
        assert ei.value.code == 1, (shift, npre)


def test_nan_count_and_quantiles_of_a_poisoned_history(demc):
    """A run from helpers.poisoned_population (NaNs of both signs, +-inf, subnormals, -0.0 in the starting states and the archive):
    nan_count is right in every pass, the NaNs are binned by their keys, and the NaN rule holds parameter by parameter."""
    from helpers import poisoned_population
    d, N, G = 5, 65, 12
    w = dict(demc.workloads.mvnormal_problem(d, N))
    w["Zinit"] = poisoned_population(d, N, 3)
    e = _engine(demc, w, N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    ch = e.get_history(1, G)[0]
    isnan = np.isnan(ch)
    assert 0 < isnan.sum() and np.signbit(ch[isnan]).any() and not np.signbit(ch[isnan]).all()
    assert isnan.any(axis=(0, 2)).any() and np.isinf(ch).any()
    zero = np.zeros((d, 1), dtype=np.uint64)
    counts, nan = e.select_counts(1, G, 56, zero)
    want, wnan = Q.count_pass(ch, 56, zero)
    assert np.array_equal(counts, want) and np.array_equal(nan, wnan) and np.array_equal(nan, isnan.sum(axis=(0, 2)))
    pre = np.array([[0x0007FFFFFFFFFF, 0xFFF80000000000]] * d, dtype=np.uint64)      # the default NaNs' keys of either sign, above their last byte
    counts, nan = e.select_counts(3, G - 1, 0, pre)
    want, wnan = Q.count_pass(ch[:, :, 2:G - 1], 0, pre)
    assert np.array_equal(counts, want) and np.array_equal(nan, wnan) and counts.sum() > 0
    hold(e.quantiles(1, G, PROBS, with_order_stats=True), Q.reference(ch), "poisoned history")
    hold(demc.quantile_chain(ch, PROBS, with_order_stats=True), Q.reference(ch), "poisoned history, array form")
    e.close()


# ---- windows inside a handle's history -------------------------------------------------------------------------------------------------
def test_windows_inside_a_history(demc, history):
    e = history
    for a, b in [(1, 130), (2, 129), (37, 101), (77, 77)]:
        ch = e.get_history(a, b)[0]
        got = e.quantiles(a, b, PROBS, with_order_stats=True)
        hold(got, Q.reference(ch), f"window {a}..{b}")
        assert np.array_equal(e.quantiles(a, b, PROBS), got.q)
        hold(demc.quantile_chain(ch, PROBS, with_order_stats=True), got, f"array form of window {a}..{b}")
    errs = []
    for f in (lambda: e.rhat(100, 131), lambda: e.quantiles(100, 131, PROBS), lambda: e.quantiles(0, 20, PROBS), lambda: e.best(100, 131),
              lambda: e.quantiles(20, 19, PROBS), lambda: e.select_counts(100, 131, 56, np.zeros((e.d, 1), dtype=np.uint64))):
        with pytest.raises(demc.DemczError) as ei:
            f()
        errs.append(ei.value.code)
    assert errs == [errs[0]] * len(errs)


def test_a_history_whose_origin_moved_twice(demc):
    d, N, G = 20, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=40)
    for g in (1, 41, 81):
        e.synchronize()
        e.set_history_origin(g - 1)
        e.run(g, g + 39, 2.38)
    for a, b in [(81, 120), (84, 118)]:
        ch, lo = e.get_history(a, b)
        hold(e.quantiles(a, b, PROBS, with_order_stats=True), Q.reference(ch), f"moved origin {a}..{b}")
        v, c, g = Q.best_reference(lo)
        best = e.best(a, b)
        assert (best.bestval, best.chain, best.generation) == (v, c, a + g) and np.array_equal(best.bestpar, ch[c, :, g])
    e.close()


def test_rhat_and_mean_cov_are_undisturbed(demc):
    """The counts and the arg-max partials lie behind R-hat's plan in the same scratch buffer, which they may have to grow."""
    d, N, G = 20, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for with_q in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G)
        e.run(1, G, 2.38)
        if with_q:
            e.quantiles(1, G, PROBS)
            e.best(1, G)
        r1 = e.rhat(1, G)
        if with_q:
            e.quantiles(37, 101, np.linspace(0, 1, 16))
            e.best(37, 101)
        out.append((r1, e.rhat(37, 101), e.mean_cov(1, G)[0], e.mean_cov(1, G)[1]))
        e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- the sharded routes ------------------------------------------------------------------------------------------------------------
def test_three_in_process_shards(demc):
    d, N, G = 9, 129, 60
    w = demc.workloads.mvnormal_problem(d, N)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=3)
    mc, Z, runner = demc.demcz_sample(w["target"], w["Zinit"], N, 10, G, 1, [range(d)], w["eps_scale"], 2.38, verbose=False,
                                      seed=5, sharding=sh, return_runner=True)
    assert len(runner.engines) == 3
    whole = demc.quantile_chain(mc.chain, PROBS, with_order_stats=True)
    hold(whole, Q.reference(mc.chain), "array form of the sharded run")
    hold(runner.quantiles(1, G, PROBS, with_order_stats=True), whole, "3 shards 1..60")
    assert np.array_equal(runner.quantiles(1, G, PROBS), whole.q)
    hold(runner.quantiles(5, 53, PROBS, with_order_stats=True), Q.reference(mc.chain[:, :, 4:53]), "3 shards 5..53")
    for a, b in [(1, G), (5, 53), (60, 60)]:
        v, c, g = Q.best_reference(mc.log_obj[:, a - 1:b])
        best = runner.best(a, b)
        assert (best.bestval, best.chain, best.generation) == (v, c, a + g) and np.array_equal(best.bestpar, mc.chain[c, :, a - 1 + g])
    runner.close()
    rccl = demc.sampler._Runner([], demc.Sharding(rank=0, world_size=2, mode="rccl"), 10, N, d)
    with pytest.raises(NotImplementedError):
        rccl.quantiles(1, 60, PROBS)
    with pytest.raises(NotImplementedError):
        rccl.best(1, 60)


def test_one_rank_communicator_returns_the_bits_of_a_handle_without_one(demc):
    d, N, G = 20, 257, 40
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for use_comm in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G, seed=1, comm=use_comm)
        e.run(1, G, 2.38)
        out.append((e.get_history(1, G)[0], e.quantiles(1, G, PROBS, with_order_stats=True), e.quantiles(4, 38, PROBS, with_order_stats=True),
                    e.best(1, G)))
        e.close()
    assert np.array_equal(out[0][0], out[1][0])
    hold(out[1][1], out[0][1], "communicator 1..40")
    hold(out[1][2], out[0][2], "communicator 4..38")
    hold(out[1][1], Q.reference(out[1][0]), "communicator against the reference")
    assert out[0][3][:3] == out[1][3][:3] and np.array_equal(out[0][3].bestpar, out[1][3].bestpar)


# ---- the best draw -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 1026), (4100, 40)], ids=Q.ids)
def test_best_of_a_log_obj_with_ties(demc, shape):
    """Chains that reject repeat their value, so the arrays are full of ties; their maximum itself is a single entry at both shapes
    (checked), so ties AT the maximum are made here: along time in its own chain, across chains in its generation, and one
    generation earlier on a higher chain -- where the reference's column-major rule and a row-major search disagree."""
    lo = S.logobj_random(*shape)
    assert (lo[:, 1:] == lo[:, :-1]).mean() > 0.3
    v, c, g = Q.best_reference(lo)
    assert demc.best_logobj(lo) == (v, c, g)
    assert 0 < g < shape[1] - 3 and 7 < c < shape[0] - 5
    tied = np.array(lo, order="F")
    tied[c, g:g + 3] = v
    assert demc.best_logobj(tied) == (v, c, g) == Q.best_reference(tied)
    tied[[c - 4, c + 2], g] = v
    assert demc.best_logobj(tied) == (v, c - 4, g) == Q.best_reference(tied)
    tied[c + 5, g - 1] = v
    assert demc.best_logobj(tied) == (v, c + 5, g - 1) == Q.best_reference(tied)
    assert tuple(np.argwhere(tied == v)[0]) == (c - 4, g)              # (row-major: not the reference's rule)
    if shape == (65, 1026):                                            # the upper chains alone have a maximum that is held twice
        sub = np.asfortranarray(lo[32:])
        assert (sub == sub.max()).sum() == 2 and demc.best_logobj(sub) == Q.best_reference(sub)


def test_best_of_uncountable_and_nan_entries(demc):
    lo, _ = S.logobj_uncountable()
    assert demc.best_logobj(lo) == (np.inf, 1, 0) == Q.best_reference(lo)                  # +inf wins; chain 1 has it from the start
    z = np.array(lo[[0, 4]], order="F")                                                    # 0.0 and -0.0 tie: the first entry wins
    assert demc.best_logobj(z)[1:] == (0, 0) == Q.best_reference(z)[1:]
    z[0, 0] = -0.0
    v, c, g = demc.best_logobj(z)
    assert (c, g) == (0, 0) and np.signbit(v) and v == 0.0
    nan = np.full((67, 5), np.nan, order="F")
    v, c, g = demc.best_logobj(nan)
    assert np.isnan(v) and (c, g) == (-1, -1)
    nan[66, 4] = -np.inf                                                                   # anything beats NaN
    assert demc.best_logobj(nan) == (-np.inf, 66, 4)
    nan[5, 2] = -1e308
    nan[:, 0] = np.nan
    assert demc.best_logobj(nan) == (-1e308, 5, 2)


def test_best_on_a_handle(demc, history):
    e = history
    for a, b in [(1, 130), (37, 101), (77, 77)]:
        ch, lo = e.get_history(a, b)
        v, c, g = Q.best_reference(lo)
        best = e.best(a, b)
        assert (best.bestval, best.chain, best.generation) == (v, c, a + g), (a, b)
        assert np.array_equal(best.bestpar, ch[c, :, g])


def test_extract_best_on_the_annealing_script(demc):
    """test/test_anneal.jl:7-29 with extract_best (utils.jl:120-125) in place of the script's hand-written lines."""
    ndim, N, K, Ngen = 10, 5, 10, 5000
    w = demc.workloads.iso_quad_problem(ndim, 5)
    mc, _ = demc.demcz_anneal(w["target"], w["Zinit"][:10 * ndim], N, K, Ngen, 1, [range(0, ndim)], 1e-5 * np.ones(ndim), 2.38,
                              verbose=False, TN=1e-4, T0=2, seed=31953150)
    bestval, bestpar = demc.extract_best(mc)
    v, c, g = Q.best_reference(mc.log_obj)
    assert bestval == v == mc.log_obj.max() and np.array_equal(bestpar, mc.chain[c, :, g])
    assert bestval > -1e-1 and np.isclose(-np.sum((bestpar - w["mu"]) ** 2), bestval, rtol=1e-12, atol=1e-300)


# ---- the summary -----------------------------------------------------------------------------------------------------------------------
def test_posterior_summary_with_quantiles(demc):
    chain = S.world(64, 3, 260)
    s = demc.posterior_summary(chain, probs=PROBS)
    assert sorted(s) == ["converged", "ess", "mcse", "mean", "quantiles", "rhat", "sd"]
    assert np.array_equal(s["quantiles"], demc.quantile_chain(chain, PROBS)) and np.array_equal(s["quantiles"], Q.world_reference((64, 3, 260)).q)
    assert sorted(demc.posterior_summary(chain)) == ["converged", "ess", "mcse", "mean", "rhat", "sd"]
