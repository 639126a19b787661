"""The autocovariance kernel (K8, demcz_kernels_acf.h), the adaptive demcz_ess around it and their Python faces against the
extended-precision reference of ess_reference.py, on the AR(1) worlds of ess_cases.py: tile counts that are no power of two, less
than one tile, chunk boundaries around the end of a half, one chain, data 1e6 standard deviations from zero, degenerate and
contaminated data; windows inside a handle's history; the sharded and the communicator routes.  test_ess_reference.py shows
without a GPU that the tolerances leave the device arithmetic a factor of ten, that the reference's stopping decisions are a
hundred times further from flipping than the tolerance of rho -- so `pairs` and `converged` must be equal -- and that a kernel
centring on the grand mean misses.  Every test prints the largest error it saw before it asserts."""
import numpy as np
import pytest

import ess_cases as C
import ess_reference as E
import stats_cases as S

pytestmark = pytest.mark.gpu


def hold_acov(A, ref, what):
    err = E.acov_error(A, ref)
    print(f"[ess] A(t) {what}: {err:.3e}")
    assert A.shape == (ref.A.shape[0], ref.L + 1) and err <= E.ACOV_RTOL, (what, err)


def hold_ess(got, ref, what, keep=None):
    """tau, var+ within tolerance; pairs and converged equal; ess the identity of the returned tau."""
    keep = np.ones(len(ref.tau), dtype=bool) if keep is None else keep
    sub = ref._replace(tau=ref.tau[keep], pairs=ref.pairs[keep], varplus=ref.varplus[keep])
    et, ev = E.tau_error(got.tau[keep], sub), E.varplus_error(got.varplus[keep], sub)
    assert np.array_equal(got.ess, E.ess_of_tau(got.tau, ref.m * ref.n), equal_nan=True), what
    print(f"[ess] {what}: tau {et:.3e} per lag, var+ {ev:.3e}; pairs {got.pairs[keep].tolist()} converged {got.converged[keep].tolist()}")
    assert np.array_equal(got.pairs[keep], ref.pairs[keep]) and np.array_equal(got.converged[keep], ref.converged[keep]), what
    assert et <= E.TAU_ATOL_PER_LAG and ev <= E.VARPLUS_RTOL, (what, et, ev)
    assert np.array_equal(got.ess[keep], E.ess_of_tau(got.tau[keep], ref.m * ref.n)), what
    for p in np.flatnonzero(~keep & np.isfinite(got.tau)):          # (not a contaminated parameter)
        hold_undecided(got, ref, int(p), what)


def hold_undecided(got, ref, p, what):
    """A parameter of a sampled history whose reference has a pair within MARGIN of zero: the device may stop elsewhere, but only
    where the reference's pairs allow it within the bound of rho (|d rho_t| <= 4e-9, so 8e-9 for a pair), and its tau must be the
    reference's sequence summed up to the device's own stopping pair, within the tolerance of tau."""
    gp, conv = int(got.pairs[p]), int(got.converged[p])
    assert 2 * (gp + conv) - 1 <= ref.L, (what, p)
    P = [float(ref.rho[p, 2 * k] + ref.rho[p, 2 * k + 1]) for k in range(gp + conv)]
    assert all(v > -8e-9 for v in P[:gp]) and (not conv or P[gp] < 8e-9), (what, p, P)
    assert conv or 2 * gp + 3 > ref.L, (what, p)                      # (not stopped: the lags really ran out)
    tau = -1 + 2 * float(np.sum(np.minimum.accumulate(P[:gp]))) if gp else -1.0
    err = abs(got.tau[p] - tau) / (2 * gp + 1)
    print(f"[ess] {what}: parameter {p} undecided (margin {ref.margin[p]:.1e}); tau up to the device's {gp} pairs {err:.3e} per lag")
    assert err <= E.TAU_ATOL_PER_LAG, (what, p, err)


def decided(ref):
    """The parameters of a sampled history (not a world chosen for it) whose stopping decisions are MARGIN from flipping: only
    for them must pairs, converged and tau equal the reference's; the others are held by hold_undecided, and A(t) is held for every
    parameter wherever it is checked."""
    keep = ref.margin >= E.MARGIN
    assert keep.sum() >= (len(keep) + 1) // 2, ref.margin
    return keep


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- the array entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", C.WORLDS, ids=C.ids)
def test_autocov_and_ess_array(demc, w):
    chain, ref = C.world(*w), C.reference(*w)
    hold_acov(demc.autocov_chain(chain, 0), ref, C.ids(w))
    got = demc.ess_chain(chain)
    hold_ess(got, ref, C.ids(w))
    if w[2] % 2:                                                     # an odd window's last generation is never read
        assert same_bits(demc.ess_chain(S.with_dropped_sample_overwritten(chain)), got)


def test_max_lag(demc):
    w = (64, 3, 260)                                                 # n = 130; pairs (1, 13, 65), the last with the lags run out
    chain = C.world(*w)
    full = C.reference(*w)
    for max_lag in (1, 129, 500, 20):                                # one pair; L; clipped to n - 1; cuts parameter 1 before it stops
        ref = C.reference(*w, max_lag)
        assert ref.L == min(129, max_lag)
        hold_ess(demc.ess_chain(chain, max_lag=max_lag), ref, f"max_lag {max_lag}")
        hold_acov(demc.autocov_chain(chain, max_lag), ref, f"max_lag {max_lag}")
    assert same_bits(demc.ess_chain(chain, max_lag=500), demc.ess_chain(chain)) and same_bits(demc.ess_chain(chain, max_lag=129), demc.ess_chain(chain))
    assert full.converged[1] == 1 and C.reference(*w, 20).converged[1] == 0 and demc.ess_chain(chain, max_lag=20).converged[1] == 0
    # a lag's sum does not depend on the lags it is computed with
    sums = demc.autocov_sums_chain(chain, 0, 129)
    for a, b in [(1, 129), (31, 33), (32, 64), (100, 100), (129, 129)]:
        assert np.array_equal(demc.autocov_sums_chain(chain, a, b), sums[:, a:b + 1]), (a, b)
    for a, b in [(-1, 3), (5, 4), (0, 130)]:
        with pytest.raises(demc.DemczError) as ei:
            demc.autocov_sums_chain(chain, a, b)
        assert ei.value.code == 1


@pytest.mark.parametrize("w", [(3, 6, 2051), (64, 3, 260), (65, 7, 20)], ids=C.ids)
def test_adaptive_route_on_arrays(demc, w):
    """(3, 6, 2051): every parameter stops, the last behind lag 165 -- two batches of 128 lags instead of 1025 lags.  The finisher
    on ONE call over all L lags must stop where the adaptive loop stopped.  (`between` is formed here in float64 from data
    centred on chain 0's first sample; the library forms it from the device's split-chain means, so tau is compared to the
    tolerance, not in bits -- the handle test below has the device's own `between` and compares bits.)"""
    N, d, G = w
    chain, ref = C.world(*w), C.reference(*w)
    n, m = G // 2, 2 * N
    sums = demc.autocov_sums_chain(chain, 0, n - 1)
    assert np.array_equal(demc.autocov_sums_chain(chain, 0, n - 1), sums)
    got = demc.ess_chain(chain)
    assert same_bits(demc.ess_chain(chain), got)                      # two identical calls return identical bits
    c = chain[:, :, :2 * n] - chain[:1, :, :1]
    means = np.concatenate([c[:, :, :n], c[:, :, n:]], axis=0).mean(axis=2)
    one = demc.ess_from_sums(m, n, sums, ((means - means.mean(axis=0)) ** 2).sum(axis=0))
    assert np.array_equal(one.pairs, got.pairs) and np.array_equal(one.converged, got.converged)
    hold_ess(one, ref, f"finisher on all lags {C.ids(w)}")


def test_adaptive_route_on_a_handle_gives_the_bits_of_all_lags(demc):
    """autocov_sums over all L lags in one call and R-hat's own stage-1 `between`, through the finisher, give the bits of ess(),
    which stopped asking for lags as soon as every parameter had stopped: a window of 2000 generations behind a burn-in of 2000
    has n = 1000 samples per split chain -- eight batches of 128 lags, of which a chain that mixes needs the first few."""
    d, N, G, a = 5, 64, 4000, 2001
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=G, seed=3)
    e.run(1, G, 2.38)
    n, m = (G - a + 1) // 2, 2 * N
    got = e.ess(a, G)
    print(f"[ess] handle 64x5, generations {a}..{G}: lags needed {(2 * got.pairs + 2).tolist()} of {n}, converged {got.converged.tolist()}, "
          f"tau {np.round(got.tau, 1).tolist()}")
    assert got.converged.all() and 2 * got.pairs.max() + 2 <= n // 2     # (else the early stop is not what is tested)
    assert same_bits(e.ess(a, G), got)
    sums = e.autocov_sums(a, G, 0, n - 1)
    s0 = e.rhat_partial(a, G, 0, None)
    s1 = e.rhat_partial(a, G, 1, s0 / m)
    assert same_bits(demc.ess_from_sums(m, n, sums, s1[:d]), got)
    ch = e.get_history(a, G)[0]
    assert same_bits(demc.ess_chain(ch), got)                         # and the array form of the same data
    ref = E.ess(ch, max_lag=2 * int(got.pairs.max()) + 1)             # (the reference up to the last stopping pair: it must stop there too)
    hold_ess(got, ref, "handle 64x5", decided(ref))
    for max_lag in (1, 31, 127, 128, 300):                            # one pair; inside a tile; a batch boundary, one past it; the third batch
        cut = e.ess(a, G, max_lag)
        assert same_bits(demc.ess_from_sums(m, n, sums[:, :max_lag + 1], s1[:d]), cut), max_lag
    e.close()


def test_degenerate_data(demc):
    got = demc.ess_chain(S.all_identical())
    assert np.isnan(got.ess).all() and np.isnan(got.tau).all() and (got.varplus == 0).all()
    assert (got.pairs == 0).all() and (got.converged == 1).all()
    # constant in time, chains differ: A(t) = 0 exactly and var+ > 0, so rho_t = 1 at every lag: every pair is 2, the lags run
    # out, tau = -1 + 2 (2 pairs) and ESS = S / (4 pairs - 1)
    c = S.constant_in_time()
    N, d, G = c.shape
    got = demc.ess_chain(c)
    assert np.array_equal(demc.autocov_chain(c, 0), np.zeros((d, G // 2))) and (got.varplus > 0).all()
    assert (got.pairs == G // 4).all() and (got.converged == 0).all()
    assert np.array_equal(got.tau, np.full(d, 4.0 * (G // 4) - 1)) and np.array_equal(got.ess, 2 * N * (G // 2) / got.tau)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_poisoned_sample_spoils_its_own_parameter_only(demc, value):
    w = (257, 6, 131)
    bad, p = C.poisoned(value, w)
    keep = np.arange(w[1]) != p
    ref = C.reference(*w)
    got = demc.ess_chain(bad)
    assert not np.isfinite(got.ess[p]) and not np.isfinite(got.tau[p]) and not np.isfinite(got.varplus[p])
    hold_ess(got, ref, f"contaminated {value}", keep)
    A = demc.autocov_chain(bad, 0)
    assert not np.isfinite(A[p]).any()
    err = E.acov_error(A[keep], ref._replace(A=ref.A[keep]))
    print(f"[ess] A(t) contaminated {value}: {err:.3e}")
    assert err <= E.ACOV_RTOL
    summary = demc.posterior_summary(bad)
    assert not np.isfinite(summary["mcse"][p]) and np.isfinite(summary["mcse"][keep]).all()


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
    ch, _ = e.get_history(a, b)
    ref = E.ess(ch)
    hold_ess(e.ess(a, b), ref, what, decided(ref))
    n = (b - a + 1) // 2
    sums = e.autocov_sums(a, b, 0, n - 1)
    hold_acov(sums / (ref.m * n), ref, what)
    return sums


def test_windows_inside_a_history(demc):
    d, N, G = 20, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, G, Gcap=G)
    e.run(1, G, 2.38)
    for a, b in [(1, 130), (2, 129), (37, 101)]:
        _hold_window(e, a, b, f"window {a}..{b}")
    with pytest.raises(demc.DemczError) as ei:
        e.ess(5, 7)                                                  # fewer than 4 generations
    assert ei.value.code == 1
    with pytest.raises(demc.DemczError) as ei:
        e.autocov_sums(5, 7, 0, 0)
    assert ei.value.code == 1
    errs = []
    for f in (lambda: e.rhat(100, 131), lambda: e.ess(100, 131), lambda: e.autocov_sums(0, 20, 0, 1)):
        with pytest.raises(demc.DemczError) as ei:
            f()                                                      # outside the history
        errs.append(ei.value.code)
    assert errs == [errs[0]] * 3
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


def test_rhat_after_ess_is_undisturbed(demc):
    """The autocovariance works behind R-hat's plan in the same scratch buffer, which it may have to grow."""
    d, N, G = 20, 300, 130
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for with_ess in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G)
        e.run(1, G, 2.38)
        if with_ess:
            e.ess(1, G)
        r1 = e.rhat(1, G)
        if with_ess:
            e.ess(37, 101)
        out.append((r1, e.rhat(37, 101), e.mean_cov(1, G)[1]))
        e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- the sharded routes ------------------------------------------------------------------------------------------------------------
def test_three_in_process_shards_against_the_reference(demc):
    """Per-engine autocov_sums and rhat_partial stages added on the host, then demcz_ess_from_sums (sampler._Runner.ess)."""
    d, N, G = 9, 129, 60
    w = demc.workloads.mvnormal_problem(d, N)
    sh = demc.Sharding(rank=0, world_size=1, mode="host", local_shards=3)
    mc, Z, runner = demc.demcz_sample(w["target"], w["Zinit"], N, 10, G, 1, [range(d)], w["eps_scale"], 2.38, verbose=False,
                                      seed=5, sharding=sh, return_runner=True)
    assert len(runner.engines) == 3
    for a, b in [(1, 60), (5, 53)]:
        ref = E.ess(mc.chain[:, :, a - 1:b])
        hold_ess(runner.ess(a, b), ref, f"3 shards {a}..{b}", decided(ref))
    ref = E.ess(mc.chain, max_lag=3)
    hold_ess(runner.ess(1, 60, max_lag=3), ref, "3 shards max_lag 3", decided(ref))
    runner.close()
    rccl = demc.sampler._Runner([], demc.Sharding(rank=0, world_size=2, mode="rccl"), 10, N, d)
    with pytest.raises(NotImplementedError):
        rccl.ess(1, 60)


def test_one_rank_communicator_returns_the_bits_of_a_handle_without_one(demc):
    d, N, G = 20, 257, 40
    w = demc.workloads.mvnormal_problem(d, N)
    out = []
    for use_comm in (False, True):
        e = _engine(demc, w, N, d, G, Gcap=G, seed=1, comm=use_comm)
        e.run(1, G, 2.38)
        out.append((e.get_history(1, G)[0], e.ess(1, G), e.ess(4, 38), e.autocov_sums(1, G, 0, 19)))
        e.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert same_bits(out[0][1], out[1][1]) and same_bits(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
    ref = E.ess(out[1][0])
    hold_ess(out[1][1], ref, "one-rank communicator 1..40", decided(ref))


# ---- the summary -------------------------------------------------------------------------------------------------------------------
def test_posterior_summary(demc):
    w = (257, 6, 131)
    chain = C.world(*w)
    s = demc.posterior_summary(chain)
    assert sorted(s) == ["converged", "ess", "mcse", "mean", "rhat", "sd"]
    e = demc.ess_chain(chain)
    assert np.array_equal(s["mean"], demc.mean_cov_chain(chain)[0]) and np.array_equal(s["rhat"], demc.Rhat_gelman(chain))
    assert np.array_equal(s["ess"], e.ess) and np.array_equal(s["converged"], e.converged)
    assert np.array_equal(s["mcse"], np.sqrt(e.varplus / e.ess)) and np.array_equal(s["sd"], np.sqrt(e.varplus))
    hold_ess(e, C.reference(*w), "summary")
