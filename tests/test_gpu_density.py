"""Posterior densities on the device (demcz_histogram, demcz_histogram2d, demcz_hdi and their Python faces) against the NumPy
references of tests/density_cases.py: every integer count with np.array_equal, edges and HDI ends as uint64 bit patterns, no
tolerance anywhere.  The conditions that give the worlds their meaning (wave-runs in one bin, waves spread over many bins,
draws on and next to every edge, ties and NaN widths in the HDI, two tiles or more) are checked on the references alone in
test_density_reference.py."""
import numpy as np
import pytest

import density_cases as D
import quantile_cases as Q
import stats_cases as S

pytestmark = pytest.mark.gpu


def hold(got, ref, what):
    assert np.array_equal(got.counts, ref.counts), what
    assert np.array_equal(D.bits(got.edges), D.bits(ref.edges)), what
    assert np.array_equal(got.below, ref.below) and np.array_equal(got.above, ref.above) and np.array_equal(got.nan, ref.nan), what


def hold2(got, ref, what):
    assert np.array_equal(got.counts, ref.counts) and np.array_equal(got.outside, ref.outside), what


def same_bits(a, b):
    return np.array_equal(D.bits(a), D.bits(b))


# ---- marginal histograms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", D.WORLDS, ids=D.ids)
def test_histogram_chain_on_the_worlds(demc, w):
    chain = S.world(*w)
    for nb in D.NBINS:
        hold(demc.histogram_chain(chain, nb), D.hist_reference(chain, nb), f"{w} at {nb} bins")
    got = demc.histogram_chain(chain)
    assert got.counts.shape == (w[1], 33) and (got.counts.sum(axis=1) == w[0] * w[2]).all()


@pytest.mark.parametrize("nb", D.NBINS)
def test_draws_on_and_next_to_every_edge(demc, nb):
    chain, rng = D.edge_world(nb)
    hold(demc.histogram_chain(chain, nb, rng), D.hist_reference(chain, nb, rng), f"edge world at {nb} bins")


def test_draws_outside_the_range_and_special_values(demc):
    chain, rng = D.out_of_range_world()
    for nb in (1, 33, 4096):
        hold(demc.histogram_chain(chain, nb, rng), D.hist_reference(chain, nb, rng), f"out-of-range world at {nb} bins")
    one = (-0.5, 0.75)                                                     # one (lo, hi) for every parameter
    hold(demc.histogram_chain(chain, 33, one), D.hist_reference(chain, 33, one), "one range for all")


def test_piled_constant_and_repeated_worlds(demc):
    chain, rng = D.piled_world()
    for nb in (2, 33, 256):
        hold(demc.histogram_chain(chain, nb, rng), D.hist_reference(chain, nb, rng), f"piled world at {nb} bins")
    chain = D.constant_world()
    got = demc.histogram_chain(chain, 33)
    hold(got, D.hist_reference(chain, 33), "constant parameter")
    assert got.counts[1, 16] == 65 * 4 and same_bits(got.edges[1][[0, -1]], [1000000.25 - 0.5, 1000000.25 + 0.5])
    chain = Q.repeated_world()
    hold(demc.histogram_chain(chain, 33), D.hist_reference(chain, 33), "repeated world")
    hold(demc.histogram_chain(chain, 4096), D.hist_reference(chain, 4096), "repeated world, 4096 bins")


def test_the_record(demc):
    chain = S.world(65, 9, 7)
    h = demc.histogram_chain(chain, 33)
    ref = D.hist_reference(chain, 33)
    assert np.array_equal(h.density, ref.counts / (ref.counts.sum(axis=1, keepdims=True) * np.diff(ref.edges, axis=1)))
    k = ref.counts.argmax(axis=1)
    assert np.array_equal(h.mode(), 0.5 * (ref.edges[np.arange(9), k] + ref.edges[np.arange(9), k + 1]))
    for prob in (0.5, 0.94):
        assert h.hdi(prob) == D.multimodal_reference(ref.counts, ref.edges, prob)


# ---- pairwise histograms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [(63, 2, 5), (65, 9, 7), (257, 20, 3), (5, 33, 4), (3, 2, 2051)], ids=D.ids)
def test_histogram2d_chain_on_the_worlds(demc, w):
    chain = S.world(*w)
    d = w[1]
    gen = np.random.default_rng([d, 18])
    allp = [(p, q) for p in range(d) for q in range(d) if p != q]
    pairs = [allp[i] for i in gen.permutation(len(allp))[:14]]
    for nbx, nby in D.GRIDS:
        got = demc.histogram2d_chain(chain, pairs, (nbx, nby))
        hold2(got, D.hist2d_reference(chain, pairs, nbx, nby), f"{w} at {nbx} x {nby}")
        r = D.auto_range(chain)
        for p in range(d):
            assert same_bits(got.edges[0][p], D.edges_of(*r[p], nbx)) and same_bits(got.edges[1][p], D.edges_of(*r[p], nby))
        assert np.array_equal(got.pairs, pairs)


def test_all_36_pairs_and_the_default(demc):
    chain = S.world(65, 9, 7)
    ref = D.hist2d_reference(chain, D.ALL36, 32, 32)
    hold2(demc.histogram2d_chain(chain, D.ALL36, 32), ref, "36 pairs")
    got = demc.histogram2d_chain(chain)                                    # all p < q at 32 x 32
    hold2(got, ref, "the default pairs")
    assert np.array_equal(got.pairs, D.ALL36) and got.counts.shape == (36, 32, 32)
    big = S.world(257, 20, 3)
    allp = [(p, q) for p in range(20) for q in range(p + 1, 20)]
    hold2(demc.histogram2d_chain(big), D.hist2d_reference(big, allp, 32, 32), "190 pairs")


def test_a_parameter_in_both_positions_mirrored_and_repeated_pairs(demc):
    chain = S.world(65, 9, 7)
    for nbx, nby in ((32, 17), (128, 128), (5, 3)):
        got = demc.histogram2d_chain(chain, D.MIXED_PAIRS, (nbx, nby))
        hold2(got, D.hist2d_reference(chain, D.MIXED_PAIRS, nbx, nby), f"mixed pairs at {nbx} x {nby}")
        assert np.array_equal(got.counts[0], got.counts[-1])               # the repeated pair
    sq = demc.histogram2d_chain(chain, [(0, 1), (1, 0)], 32)
    assert np.array_equal(sq.counts[0], sq.counts[1].T)                    # square grids: (q, p) is (p, q) transposed


def test_pairs_with_draws_on_edges_and_outside(demc):
    for nb in (1, 2, 33, 128):
        chain, rng = D.edge_world(nb)
        pairs = [(0, 1), (1, 0)]
        hold2(demc.histogram2d_chain(chain, pairs, nb, rng), D.hist2d_reference(chain, pairs, nb, nb, rng), f"edge world at {nb} x {nb}")
    chain, rng = D.out_of_range_world()
    pairs = [(0, 1), (2, 0), (1, 2), (2, 1)]
    for nbx, nby in D.GRIDS:
        got = demc.histogram2d_chain(chain, pairs, (nbx, nby), rng)
        hold2(got, D.hist2d_reference(chain, pairs, nbx, nby, rng), f"out-of-range world at {nbx} x {nby}")
        assert (got.outside > 0).all() and (got.counts.sum(axis=(1, 2)) + got.outside == 65 * 9).all()


# ---- highest-density intervals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", D.WORLDS, ids=D.ids)
def test_hdi_chain_on_the_worlds(demc, w):
    chain = S.world(*w)
    got = demc.hdi_chain(chain, D.HDI_PROBS)
    assert got.shape == (w[1], len(D.HDI_PROBS), 2) and same_bits(got, D.hdi_reference(chain, D.HDI_PROBS)), w
    one = demc.hdi_chain(chain)
    assert one.shape == (w[1], 2) and same_bits(one, D.hdi_reference(chain, [0.94])[:, 0, :])


def test_hdi_ties_nan_widths_and_nan_draws(demc):
    chain = D.hdi_special_world()
    ref = D.hdi_reference(chain, D.HDI_PROBS)
    assert same_bits(demc.hdi_chain(chain, D.HDI_PROBS), ref)
    for negative in (False, True):
        x = Q.with_nan(negative)
        got = demc.hdi_chain(x, D.HDI_PROBS)
        assert np.isnan(got[1]).all() and same_bits(got[[0, 2]], ref[[0, 2]]) and same_bits(got, D.hdi_reference(x, D.HDI_PROBS))
    chain = Q.repeated_world()
    sixteen = tuple(np.linspace(0.01, 0.99, 16))
    assert same_bits(demc.hdi_chain(chain, sixteen), D.hdi_reference(chain, sixteen))
    allinf = np.asfortranarray(np.full((3, 1, 2), np.inf))
    assert np.isnan(demc.hdi_chain(allinf, [0.5])).all()                   # inf - inf throughout: no candidate
    zeros = np.asfortranarray(np.array([0.0, -0.0, -0.0, 0.0, 1.0]).reshape(5, 1, 1))
    got = demc.hdi_chain(zeros, [0.5])
    assert same_bits(got, D.hdi_reference(zeros, [0.5])) and same_bits(got[0, 0], [0.0, 0.0])     # -0.0 is taken as 0.0


# ---- the handle forms ------------------------------------------------------------------------------------------------------------------
def _engine(demc, w, N, d, G, Gcap, seed=21, K=10, comm=False):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=Gcap, blockindex=[range(d)], eps_scale=w["eps_scale"],
                       seed=seed, target=w["target"])
    if comm:
        e.comm_init(e.comm_unique_id(), 1, 0)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


PAIRS9 = [(0, 1), (1, 0), (3, 8), (8, 2), (2, 3), (4, 7), (7, 5), (6, 0)]
PROBS2 = (0.5, 0.94)


def everything(h, a, b):
    """What the three calls return for a window, on anything with the statistics' methods."""
    return (h.histogram(a, b, 33), h.histogram(a, b, 4096), h.histogram2d(a, b, PAIRS9, (32, 17)), h.hdi(a, b, PROBS2))


def hold_everything(got, ch, what, rng=None):
    hold(got[0], D.hist_reference(ch, 33, rng), what)
    hold(got[1], D.hist_reference(ch, 4096, rng), what)
    hold2(got[2], D.hist2d_reference(ch, PAIRS9, 32, 17, rng), what)
    assert same_bits(got[3], D.hdi_reference(ch, PROBS2)), what


def everything_chain(demc, ch):
    return (demc.histogram_chain(ch, 33), demc.histogram_chain(ch, 4096), demc.histogram2d_chain(ch, PAIRS9, (32, 17)),
            demc.hdi_chain(ch, PROBS2))


@pytest.fixture(scope="module")
def history(demc):
    """One engine with 130 generations of a d = 9, N = 300 run, shared by the tests that only read it."""
    d, N, G = 9, 300, 130
    e = _engine(demc, demc.workloads.mvnormal_problem(d, N), N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    yield e
    e.close()


def test_windows_inside_a_history_and_the_array_forms(demc, history):
    e = history
    for a, b in [(1, 130), (37, 101), (77, 77)]:
        ch = e.get_history(a, b)[0]
        got = everything(e, a, b)
        hold_everything(got, ch, f"window {a}..{b}")
        arr = everything_chain(demc, ch)
        hold(arr[0], got[0], "array form")
        hold(arr[1], got[1], "array form")
        hold2(arr[2], got[2], "array form")
        assert same_bits(arr[3], got[3])
    ch = e.get_history(37, 101)[0]
    rng = np.percentile(ch, [10, 80], axis=(0, 2)).T
    hold(e.histogram(37, 101, 33, rng), D.hist_reference(ch, 33, rng), "a given range")
    hold2(e.histogram2d(37, 101, PAIRS9, 32, rng), D.hist2d_reference(ch, PAIRS9, 32, 32, rng), "a given range")
    hold2(e.histogram2d(37, 101), D.hist2d_reference(ch, D.ALL36, 32, 32), "the default pairs")
    assert same_bits(e.hdi(37, 101), D.hdi_reference(ch, [0.94])[:, 0, :])


def test_a_history_whose_origin_moved(demc):
    d, N, G = 9, 129, 120
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=40)
    for g in (1, 41, 81):
        e.synchronize()
        e.set_history_origin(g - 1)
        e.run(g, g + 39, 2.38)
    for a, b in [(81, 120), (84, 118)]:
        hold_everything(everything(e, a, b), e.get_history(a, b)[0], f"moved origin {a}..{b}")
    e.close()


def test_a_derived_history(demc):
    chain = S.world(65, 9, 7)
    with demc.rank_normalize_chain(chain) as h:                            # the normal scores: a DerivedHistory, generations 1..7
        z = h.get()
        hold_everything(everything(h, 1, 7), z, "derived history")
        hold_everything(everything(h, 2, 6), z[:, :, 1:6], "window of a derived history")
        s = h.summary(hdi_prob=0.9)
        assert same_bits(s["hdi"], D.hdi_reference(z, [0.9])[:, 0, :])
        assert sorted(h.summary()) == sorted(set(s) - {"hdi"})


# ---- the sharded routes ----------------------------------------------------------------------------------------------------------------
def test_three_in_process_shards(demc):
    d, N, G = 9, 129, 60
    w = demc.workloads.mvnormal_problem(d, N)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=3)
    mc, Z, runner = demc.demcz_sample(w["target"], w["Zinit"], N, 10, G, 1, [range(d)], w["eps_scale"], 2.38, verbose=False,
                                      seed=5, sharding=sh, return_runner=True)
    assert len(runner.engines) == 3
    for a, b in [(1, G), (5, 53)]:
        ch = mc.chain[:, :, a - 1:b]
        hold(runner.histogram(a, b, 33), D.hist_reference(ch, 33), f"3 shards {a}..{b}")          # the extremes over the shards
        hold(runner.histogram(a, b), demc.histogram_chain(ch), "3 shards against the array form")
        hold2(runner.histogram2d(a, b, PAIRS9, (32, 17)), D.hist2d_reference(ch, PAIRS9, 32, 17), f"3 shards {a}..{b}")
        rng = np.percentile(ch, [10, 80], axis=(0, 2)).T
        hold(runner.histogram(a, b, 256, rng), D.hist_reference(ch, 256, rng), "3 shards, a given range")
        hold2(runner.histogram2d(a, b, None, 32, rng), D.hist2d_reference(ch, D.ALL36, 32, 32, rng), "3 shards, a given range")
    with pytest.raises(NotImplementedError):
        runner.hdi(1, G)
    runner.close()
    rccl = demc.sampler._Runner([], demc.Sharding(rank=0, world_size=2, mode="rccl"), 10, N, d)
    for f in (lambda: rccl.histogram(1, 60), lambda: rccl.histogram2d(1, 60), lambda: rccl.hdi(1, 60)):
        with pytest.raises(NotImplementedError):
            f()


def test_one_rank_communicator_returns_the_bits_of_a_handle_without_one(demc):
    d, N, G = 9, 257, 40
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for use_comm in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G, seed=1, comm=use_comm)
        e.run(1, G, 2.38)
        out.append((e.get_history(1, G)[0], everything(e, 1, G), everything(e, 4, 38)))
        e.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in (1, 2):
        hold(out[1][k][0], out[0][k][0], "communicator")
        hold(out[1][k][1], out[0][k][1], "communicator")
        hold2(out[1][k][2], out[0][k][2], "communicator")
        assert same_bits(out[1][k][3], out[0][k][3])
    hold_everything(out[1][1], out[1][0], "communicator against the reference")


# ---- the summary -----------------------------------------------------------------------------------------------------------------------
def test_posterior_summary_with_hdi(demc):
    chain = S.world(64, 3, 260)
    s = demc.posterior_summary(chain, hdi_prob=0.9)
    assert sorted(s) == ["converged", "ess", "hdi", "mcse", "mean", "rhat", "sd"]
    assert same_bits(s["hdi"], D.hdi_reference(chain, [0.9])[:, 0, :]) and same_bits(s["hdi"], demc.hdi_chain(chain, 0.9))
    two = demc.posterior_summary(chain, hdi_prob=[0.5, 0.9])["hdi"]
    assert same_bits(two, D.hdi_reference(chain, [0.5, 0.9]))
    assert sorted(demc.posterior_summary(chain)) == ["converged", "ess", "mcse", "mean", "rhat", "sd"]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(demc, history):
    e = history
    chain = S.world(65, 3, 9)
    nan = float("nan")
    calls = {
        "0 bins": lambda: demc.histogram_chain(chain, 0),
        "4097 bins": lambda: demc.histogram_chain(chain, 4097),
        "0 bins on a handle": lambda: e.histogram(1, 130, 0),
        "4097 bins on a handle": lambda: e.histogram(1, 130, 4097),
        "129 wide": lambda: demc.histogram2d_chain(chain, None, (129, 32)),
        "129 high": lambda: demc.histogram2d_chain(chain, None, (32, 129)),
        "0 wide": lambda: e.histogram2d(1, 130, None, (0, 32)),
        "lo == hi": lambda: demc.histogram_chain(chain, 33, (1.0, 1.0)),
        "lo > hi": lambda: demc.histogram_chain(chain, 33, [(0.0, 1.0), (2.0, 1.0), (0.0, 1.0)]),
        "NaN range": lambda: demc.histogram_chain(chain, 33, (nan, 1.0)),
        "NaN range 2d": lambda: demc.histogram2d_chain(chain, None, 32, (0.0, nan)),
        "infinite range": lambda: e.histogram(1, 130, 33, (-np.inf, 1.0)),
        "(p, p)": lambda: demc.histogram2d_chain(chain, [(0, 1), (1, 1)]),
        "pair out of range": lambda: demc.histogram2d_chain(chain, [(0, 3)]),
        "negative pair": lambda: e.histogram2d(1, 130, [(-1, 0)]),
        "prob 0": lambda: demc.hdi_chain(chain, 0.0),
        "prob 1": lambda: e.hdi(1, 130, 1.0),
        "prob NaN": lambda: demc.hdi_chain(chain, [0.5, nan]),
        "17 probabilities": lambda: demc.hdi_chain(chain, np.linspace(0.1, 0.9, 17)),
        "no probability": lambda: e.hdi(1, 130, []),
        "a NaN draw under an automatic range": lambda: demc.histogram_chain(Q.with_nan(False), 33),
        "an infinite draw under an automatic range": lambda: demc.histogram2d_chain(Q.specials(), [(1, 2)]),
    }
    for what, f in calls.items():
        with pytest.raises(demc.DemczError) as ei:
            f()
        assert ei.value.code == 1, what
    poisoned = np.array(chain, order="F")
    poisoned[33, 1, 5] = -nan
    with pytest.raises(demc.DemczError) as ei:
        demc.histogram_chain(poisoned, 33)
    assert ei.value.code == 1 and "parameter 1" in str(ei.value)           # the message names the poisoned parameter
    with pytest.raises(demc.DemczError) as ei:
        demc.histogram_chain(Q.specials(), 33)
    assert "parameter 0" in str(ei.value)
    # a window outside the history: the code of every other statistic
    errs = []
    for f in (lambda: e.rhat(100, 131), lambda: e.histogram(100, 131), lambda: e.histogram(0, 20), lambda: e.histogram2d(100, 131),
              lambda: e.hdi(100, 131), lambda: e.hdi(20, 19), lambda: e.histogram(100, 131, 33, (0.0, 1.0))):
        with pytest.raises(demc.DemczError) as ei:
            f()
        errs.append(ei.value.code)
    assert errs == [errs[0]] * len(errs)
    # ... and after all of them the handle still answers
    hold(e.histogram(77, 77, 33), D.hist_reference(e.get_history(77, 77)[0], 33), "after the refusals")


def test_a_poisoned_history_under_an_automatic_and_a_given_range(demc):
    from helpers import poisoned_population
    d, N, G = 5, 65, 12
    w = dict(demc.workloads.mvnormal_problem(d, N))
    w["Zinit"] = poisoned_population(d, N, 3)
    e = _engine(demc, w, N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    ch = e.get_history(1, G)[0]
    assert np.isnan(ch).any() and np.isinf(ch).any()
    for f in (lambda: e.histogram(1, G), lambda: e.histogram2d(1, G)):
        with pytest.raises(demc.DemczError) as ei:
            f()
        assert ei.value.code == 1 and "parameter" in str(ei.value)
    rng = (-3.0, 3.0)
    got = e.histogram(1, G, 33, rng)
    hold(got, D.hist_reference(ch, 33, rng), "poisoned history, a given range")
    assert got.nan.sum() == np.isnan(ch).sum() > 0
    hold2(e.histogram2d(1, G, None, (32, 17), rng), D.hist2d_reference(ch, [(p, q) for p in range(d) for q in range(p + 1, d)], 32, 17, rng),
          "poisoned history, a given range")
    assert same_bits(e.hdi(1, G, PROBS2), D.hdi_reference(ch, PROBS2))
    e.close()


# ---- the neighbours --------------------------------------------------------------------------------------------------------------------
def test_the_other_statistics_are_undisturbed(demc):
    """The counts lie behind R-hat's plan in the handle's scratch buffer, which they may have to grow, and the HDI shares the
    ranks' sort: rhat, mean_cov, quantiles and rank_diagnostics return the same bits with and without the new calls between them."""
    d, N, G = 9, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for with_new in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G)
        e.run(1, G, 2.38)
        if with_new:
            everything(e, 1, G)
        first = (e.rhat(1, G), e.quantiles(1, G, Q.PROBS), *e.rank_diagnostics(1, G))
        if with_new:
            everything(e, 37, 101)
            e.histogram2d(1, G, None, 128)
        out.append(first + (e.rhat(37, 101), *e.mean_cov(1, G), e.quantiles(37, 101, Q.PROBS), *e.rank_diagnostics(37, 101)))
        if with_new:
            hold_everything(everything(e, 1, G), e.get_history(1, G)[0], "after the other statistics")
        e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)
