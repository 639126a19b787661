"""CPU tier of the snooker update: the worlds of tests/snooker_cases.py are worth running, the pieces of the reference step
(tests/snooker_reference.py) are what the spec says, and the step samples the right distribution -- from the reference alone.

  * every world shows accepted and rejected snooker steps; the marked worlds show steps whose norms are no positive normal
    doubles (e2 == 0 from a chain that meets its own row; infinite and NaN norms from +-inf in the archive); the tempered world
    has T = 0 at snooker and at ordinary generations;
  * the anchor is never one of the two projected rows and is uniform over the others (exhaustive at M = 3, 4, 5);
  * gamma_s stays within its bounds, ends included;
  * a run cut into pieces is the run in one piece (the reference's own cut rule);
  * the moment test: the step as the only move on a correlated Gaussian recovers mean and covariance, and does not with the
    Jacobian left out or with its exponent one off in either direction."""
import math

import numpy as np
import pytest

import snooker_cases as sc
import snooker_reference as sr
from helpers import same_bits


@pytest.mark.parametrize("name", list(sc.WORLDS))
def test_every_world_shows_both_outcomes(oracle, name):
    w, ref, run = sc.reference(oracle, name)
    facts = [f for _, _, f in run.steps]
    assert len(run.snooker_generations) == sum(1 for g in range(1, w["G"] + 1) if g % w["every"] == 0)
    assert len(facts) == w["N"] * len(run.snooker_generations)
    assert sum(f["accepted"] for f in facts) >= 10 and sum(f["valid"] and not f["accepted"] for f in facts) >= 10, name
    assert all(f["ia"] not in (f["i1"], f["i2"]) and f["i1"] != f["i2"] for f in facts)
    assert all(sc.GAMMA_S[0] <= f["gamma_s"] <= sc.GAMMA_S[1] for f in facts)
    # the part-filled wave has snooker steps of both outcomes too
    assert {f["accepted"] for (_, c, f) in run.steps if c >= 64} == {True, False}, name
    if w["needs_invalid"]:
        assert sum(not f["valid"] for f in facts) >= 3, name
    assert ref["M"] == w["Z0"].shape[0] + w["N"] * (w["G"] // w["K"])


def test_the_marked_worlds_are_invalid_in_the_ways_they_claim(oracle):
    _, _, own = sc.reference(oracle, "mvn5_own_row")
    assert sum(f["e2"] == 0.0 for _, _, f in own.steps) >= 3
    _, ref, inf = sc.reference(oracle, "iso6_inf")
    e2 = [f["e2"] for _, _, f in inf.steps]
    f2 = [f.get("f2", 1.0) for _, _, f in inf.steps]
    assert any(math.isinf(v) for v in e2) and any(math.isnan(v) or math.isinf(v) for v in f2)
    assert np.isfinite(ref["chain"][:, :, [g - 1 for g in inf.snooker_generations]]).all(), "an invalid step's proposal must not reach the state"


def test_the_tempered_world_has_zero_temperatures_at_both_kinds_of_generation(oracle):
    w, _, run = sc.reference(oracle, "mvn5_tempered")
    T = w["temperature"]
    sn = set(run.snooker_generations)
    assert any(T[g - 1] == 0.0 for g in sn) and any(T[g - 1] == 0.0 for g in range(1, w["G"] + 1) if g not in sn)
    assert {0.0, 1e-300, 1e300} <= {T[g - 1] for g in sn}
    plain = sc.mixed_run(oracle, w)
    plain.run(1, w["G"], w["gamma"], None)
    assert not np.array_equal(plain.result()["chain"], sc.reference(oracle, "mvn5_tempered")[1]["chain"])


@pytest.mark.parametrize("M", [3, 4, 5])
def test_the_anchor_is_uniform_over_the_other_rows(M):
    grid = [(k * (1 << 64)) // 60 + 12345 for k in range(60)]        # 60 = lcm(1, 2, 3) * 20 words, evenly spread
    for i1 in range(M):
        for i2 in range(M):
            if i1 == i2:
                continue
            got = [sr.anchor_index(r, M, i1, i2) for r in grid]
            assert set(got) == set(range(M)) - {i1, i2}
            assert all(got.count(j) == 60 // (M - 2) for j in set(got)), (M, i1, i2)
            assert got == sorted(got)                                  # monotone in the word
    assert sr.anchor_index((1 << 64) - 1, 1000, 998, 999) == 997 and sr.anchor_index(0, 1000, 0, 1) == 2
    assert sr.anchor_index((1 << 64) - 1, 1000, 5, 999) == 998 and sr.anchor_index(0, 1000, 1, 0) == 2


def test_gamma_s_stays_within_its_bounds():
    for lo, hi in ((1.2, 2.2), (0.5, 0.5), (1e-3, 1e3)):
        for r in (0, 1, (1 << 12) - 1, 1 << 63, (1 << 64) - 1):
            assert lo <= sr.gamma_s(r, lo, hi) <= hi
    assert sr.u_open(0) == 2.0 ** -53 and sr.u_open((1 << 64) - 1) == 1.0 - 2.0 ** -53


def test_a_reference_run_in_pieces_is_the_run_in_one(oracle):
    for name, cuts in (("mvn7", [2, 3, 4, 13, 30, 31, 40]), ("rosenbrock7", [9, 10, 25, 40])):
        w, ref, _ = sc.reference(oracle, name)
        run = sc.mixed_run(oracle, w)
        a = 1
        for b in cuts:
            run.run(a, b, w["gamma"], None)
            a = b + 1
        same_bits(run.result(), ref, what=name)


def test_a_resumed_reference_follows_the_streams(oracle):
    """rng_offset = 20 with every = 3: the second part's snooker generations are those of the whole run, not its own multiples."""
    w, ref, whole = sc.reference(oracle, "mvn7")
    first = sc.mixed_run(oracle, w)
    first.run(1, 20, w["gamma"])
    r1 = first.result()
    second = sc.mixed_run(oracle, w, Z0=r1["Z"], X0=r1["X"], lp0=r1["logp"], rng_offset=20)
    second.run(1, 20, w["gamma"])
    assert [g + 20 for g in second.snooker_generations] == [g for g in whole.snooker_generations if g > 20] != [g for g in range(21, 41) if (g - 20) % 3 == 0]
    r2 = second.result()
    assert np.array_equal(r2["chain"][:, :, :20], ref["chain"][:, :, 20:]) and np.array_equal(r2["Z"], ref["Z"])


def test_the_drivers_refuse_before_they_build_an_engine(demc):
    """snooker_every > 0: a layout other than the one-lane one, a Python closure, an engine without set_snooker, two archive rows."""
    from oracle_engine import OracleEngine
    w = demc.workloads.mvnormal_problem(5, 8)
    args = (w["Zinit"], 8, 10, 20, 1, [range(5)], w["eps_scale"], w["gamma"])
    for driver in (demc.demcz_sample, demc.demcz_anneal):
        with pytest.raises(ValueError, match="one-lane"):
            driver(w["target"], *args, verbose=False, snooker_every=5, lanes_per_chain=16)
        with pytest.raises(ValueError, match="device target"):
            driver(lambda x: -float(np.sum(x * x)), *args, verbose=False, snooker_every=5)
        with pytest.raises(ValueError, match="set_snooker"):
            driver(w["target"], *args, verbose=False, snooker_every=5, engine_factory=OracleEngine)
        with pytest.raises(ValueError, match=">= 0"):
            driver(w["target"], *args, verbose=False, snooker_every=-1)
    with pytest.raises(ValueError, match="3 rows"):
        demc.demcz_sample(w["target"], w["Zinit"][:2], 2, 10, 20, 1, [range(5)], w["eps_scale"], w["gamma"], verbose=False, snooker_every=5)
    # every = 0 leaves the drivers as they were: the oracle-backed engine runs
    mc, _ = demc.demcz_sample(w["target"], *args, verbose=False, snooker_every=0, engine_factory=OracleEngine)
    assert mc.chain.shape == (8, 5, 20)
    assert len(demc.DEMCopt.__dataclass_fields__) == 14


# ---- the moment test ---------------------------------------------------------------------------------------------------------------
D, CHAINS, GENS, KEEP_FROM, K = 5, 64, 6000, 2000, 10


def _moments(jac_power, seed=20081216):
    """The snooker step as the only move: 64 chains, 6000 generations, an archive of 10 d overdispersed rows that takes the
    population in every K-th generation; mean and covariance of the last two thirds."""
    rng = np.random.default_rng(seed)
    idx = np.arange(D)
    Sigma = 0.7 ** np.abs(idx[:, None] - idx[None, :])           # unit variances (the mean's bound is absolute), neighbours at 0.7
    mu = np.linspace(-1.0, 1.0, D)
    P = np.linalg.inv(Sigma)
    logp = lambda X: -0.5 * np.einsum("ni,ij,nj->n", X - mu, P, X - mu)
    L = np.linalg.cholesky(Sigma)
    Z = np.empty((10 * D + CHAINS * (GENS // K), D))
    M = 10 * D
    Z[:M] = mu + 2.0 * rng.standard_normal((M, D)) @ L.T
    X = mu + 2.0 * rng.standard_normal((CHAINS, D)) @ L.T
    lp = logp(X)
    kept = np.empty((GENS - KEEP_FROM, CHAINS, D))
    for g in range(1, GENS + 1):
        X, lp = sr.snooker_population_step(rng, X, lp, Z[:M], logp, sc.GAMMA_S, jac_power)
        if g > KEEP_FROM:
            kept[g - KEEP_FROM - 1] = X
        if g % K == 0:
            Z[M:M + CHAINS] = X
            M += CHAINS
    flat = kept.reshape(-1, D)
    cov = np.cov(flat, rowvar=False)
    return float(np.abs(cov - Sigma).max() / np.abs(Sigma).max()), float(np.abs(flat.mean(axis=0) - mu).max())


def test_the_step_samples_the_target_and_its_wrong_forms_do_not():
    cov_err, mean_err = _moments(None)
    print(f"exponent d - 1: covariance {cov_err:.4f}, mean {mean_err:.4f}")
    assert cov_err < 0.08 and mean_err < 0.1
    for what, power in (("no Jacobian", -math.inf), ("exponent d", D), ("exponent d - 2", D - 2)):
        wrong, _ = _moments(power)
        print(f"{what}: covariance {wrong:.4f}")
        assert not wrong < 0.08, what
