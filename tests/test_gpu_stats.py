"""The statistics kernels (K5 split R-hat, K7a accept ratio, K7b mean / covariance) and their host halves against the
extended-precision reference of stats_reference.py, on the inputs of stats_cases.py: every tile count of the covariance, chain
counts around one workgroup, chunk lengths that do not divide the window, empty chunks, data 1e6 standard deviations from zero,
degenerate and contaminated data; windows inside a handle's history; the sharded and the communicator routes; the monitor of
demcz_run_checked.  test_stats_reference.py shows without a GPU that the tolerances leave a correct float64 kernel a factor of
ten and that one without the shift by a first sample misses them by more than a hundred.  Every test prints the largest error it
saw before it asserts."""
import numpy as np
import pytest

import stats_cases as S
import stats_reference as R

pytestmark = pytest.mark.gpu
ids = lambda w: "x".join(str(v) for v in w)      # noqa: E731
RHAT_CASES = [w for w in S.all_worlds() if S.has_rhat(w)]


def hold_rhat(got, ref, what):
    err = R.rhat_error(got, ref)
    print(f"[stats] rhat {what}: {err:.3e}")
    assert err <= R.RHAT_RTOL, (what, err)


def hold_mean_cov(mean, cov, ref_mean, ref_cov, what):
    em, ec = R.mean_error(mean, ref_mean, ref_cov), R.cov_error(cov, ref_cov)
    print(f"[stats] mean {what}: {em:.3e}   cov {what}: {ec:.3e}")
    assert em <= R.MEAN_RTOL and ec <= R.COV_RTOL, (what, em, ec)
    assert np.array_equal(cov, cov.T), f"{what}: the two triangles come from the same accumulator"


# ---- the array entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", S.all_worlds(), ids=ids)
def test_mean_cov_array(demc, w):
    mean, cov = demc.mean_cov_chain(S.world(*w))
    hold_mean_cov(mean, cov, *S.meancov_reference(*w), what=ids(w))


def test_mean_cov_of_one_sample_is_exact(demc):
    one = S.world(*S.MEANCOV_EXACT)
    mean, cov = demc.mean_cov_chain(one)
    assert np.array_equal(mean, one[0, :, 0]) and np.array_equal(cov, np.zeros((3, 3)))


@pytest.mark.parametrize("w", RHAT_CASES, ids=ids)
def test_rhat_array(demc, w):
    """Rhat_gelman, and the same through convergence_check beside an accept ratio of the same shape; an odd window's last
    generation is never read."""
    N, d, G = w
    chain, lo = S.world(*w), S.logobj_random(N, G)
    rh = demc.Rhat_gelman(chain)
    hold_rhat(rh, S.rhat_reference(*w), ids(w))
    acc, rh2 = demc.convergence_check(chain, lo, verbose=False)
    assert np.array_equal(rh2, rh) and np.array_equal(acc, R.accept_ratio(lo))
    if G % 2:
        assert np.array_equal(demc.Rhat_gelman(S.with_dropped_sample_overwritten(chain)), rh)


def test_rhat_of_degenerate_data(demc):
    """W = 0: the shifted sums are exactly zero, so +inf where the chains differ from each other and nan where nothing does."""
    assert np.isposinf(demc.Rhat_gelman(S.constant_in_time())).all()
    assert np.isnan(demc.Rhat_gelman(S.all_identical())).all()
    mean, cov = demc.mean_cov_chain(S.all_identical())
    assert np.array_equal(mean, np.full(3, 1000000.25)) and np.array_equal(cov, np.zeros((3, 3)))


@pytest.mark.parametrize("N,G", S.ACCEPT_SHAPES)
def test_accept_ratio_array(demc, N, G):
    """Equality: both sides divide the same two exact integers once."""
    for what, lo in (("random", S.logobj_random(N, G)), ("chunk ends", S.logobj_on_chunk_boundaries(N, G, 0)),
                     ("chunk starts", S.logobj_on_chunk_boundaries(N, G, 1))):
        got, ref = demc.accept_ratio(lo), R.accept_ratio(lo)
        assert np.array_equal(got, ref), (what, int(np.count_nonzero(got != ref)), (got - ref)[got != ref][:4] * (G - 1))
    if N > 1:
        r = demc.accept_ratio(S.logobj_random(N, G))
        assert r[0] == 1.0 and r[-1] == 0.0


def test_accept_ratio_of_pairs_that_are_not_what_they_look_like(demc):
    lo, expect = S.logobj_uncountable()
    assert np.array_equal(demc.accept_ratio(lo), expect / np.float64(lo.shape[1] - 1))


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_poisoned_sample_spoils_its_own_parameter_only(demc, value):
    w, p = S.CONTAMINATED, S.POISON_AT[1]
    d = w[1]
    bad = S.contaminated(value)
    keep = np.arange(d) != p
    rh = demc.Rhat_gelman(bad)
    assert not np.isfinite(rh[p])
    hold_rhat(rh[keep], S.rhat_reference(*w)[keep], f"contaminated {value}")
    mean, cov = demc.mean_cov_chain(bad)
    assert not np.isfinite(mean[p]) and not np.isfinite(cov[p, :]).any() and not np.isfinite(cov[:, p]).any()
    rm, rc = S.meancov_reference(*w)
    sub = np.ix_(keep, keep)
    hold_mean_cov(mean[keep], cov[sub], rm[keep], rc[sub], f"contaminated {value}")


# ---- windows inside a handle's history ---------------------------------------------------------------------------------------------
def _engine(demc, w, N, d, G, Gcap, seed=21, K=10, comm=False):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=Gcap, blockindex=[range(d)], eps_scale=w["eps_scale"],
                       seed=seed, target=w["target"])
    if comm:
        e.comm_init(e.comm_unique_id(), 1, 0)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


def _hold_window(e, a, b, what):
    ch, lo = e.get_history(a, b)
    hold_rhat(e.rhat(a, b), R.rhat_gelman(ch), what)
    mean, cov = e.mean_cov(a, b)
    hold_mean_cov(mean, cov, *R.mean_cov_chain(ch), what=what)
    assert np.array_equal(e.accept_ratio(a, b), R.accept_ratio(lo)), what


def test_windows_inside_a_history(demc):
    d, N, G = 20, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    for a, b in [(1, 130), (2, 129), (37, 101), (127, 130)]:
        _hold_window(e, a, b, f"window {a}..{b}")
    with pytest.raises(demc.DemczError) as ei:
        e.rhat(5, 7)                                                 # fewer than 4 generations
    assert ei.value.code == 1
    with pytest.raises(demc.DemczError) as ei:
        e.accept_ratio(9, 9)                                         # fewer than 2
    assert ei.value.code == 1
    e.close()
    # a history of 40 generations whose origin has moved twice
    e = _engine(demc, w, N, d, G, Gcap=40)
    for g in (1, 41, 81):
        e.synchronize()
        e.set_history_origin(g - 1)
        e.run(g, g + 39, 2.38)
    for a, b in [(81, 120), (84, 118)]:
        _hold_window(e, a, b, f"moved origin {a}..{b}")
    e.close()


# ---- the sharded routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N", [(9, 129), (20, 258)])
def test_three_in_process_shards_against_the_reference(demc, d, N):
    """demcz_rhat_partial stage 0 / 1 of three shards combined on the host (sampler._Runner.rhat)."""
    G = 60
    w = demc.workloads.mvnormal_problem(d, N)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=3)
    mc, Z, runner = demc.demcz_sample(w["target"], w["Zinit"], N, 10, G, 1, [range(d)], w["eps_scale"], 2.38, verbose=False,
                                      seed=5, sharding=sh, return_runner=True)
    assert len(runner.engines) == 3
    for a, b in [(1, 60), (5, 53)]:
        hold_rhat(runner.rhat(a, b), R.rhat_gelman(mc.chain[:, :, a - 1:b]), f"3 shards d={d} {a}..{b}")
    runner.close()


def test_one_rank_communicator_against_the_reference(demc):
    """rhat_reduce_kernel with the grand mean formed on the device, then rhat_final_kernel: held to the reference, and the bits of
    the one-workgroup route of a handle without a communicator."""
    d, N, G = 20, 257, 40
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for use_comm in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G, seed=1, comm=use_comm)
        e.run(1, G, 2.38)
        out.append((e.get_history(1, G)[0], e.rhat(1, G), e.rhat(4, 38)))
        e.close()
    assert np.array_equal(out[0][0], out[1][0])
    hold_rhat(out[1][1], R.rhat_gelman(out[1][0]), "one-rank communicator 1..40")
    hold_rhat(out[1][2], R.rhat_gelman(out[1][0][:, :, 3:38]), "one-rank communicator 4..38")
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# ---- the monitor ------------------------------------------------------------------------------------------------------------------
def test_monitor_values_against_the_reference(demc):
    d, N, G, every = 12, 64, 256, 64
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=G, seed=9)
    g_stop, mx, last = e.run_checked(1, G, 2.38, every, 0.0)
    assert g_stop == G and len(mx) == 4
    chain = e.get_history(1, G)[0]
    refs = [R.rhat_gelman(chain[:, :, g:g + every]) for g in range(0, G, every)]
    hold_rhat(mx, np.array([r.max() for r in refs]), "monitor max per slab")
    hold_rhat(last, refs[-1], "monitor last")
    twin = _engine(demc, w, N, d, G, Gcap=G, seed=9)
    trace = []
    for g in range(1, G, every):
        twin.run(g, g + every - 1, 2.38)
        trace.append(twin.rhat(g, g + every - 1))
    assert np.array_equal(mx, [r.max() for r in trace]) and np.array_equal(last, trace[-1])
    e.close()
    twin.close()
