"""CPU tier of the snooker update: the worlds of tests/snooker_cases.py are worth running, the pieces of the reference step
(tests/snooker_reference.py) are what the spec says, and the step samples the right distribution -- from the reference alone.

  * every world shows accepted and rejected snooker steps; the marked worlds show steps whose norms are no positive normal
    doubles (e2 == 0 from a chain that meets its own row; infinite and NaN norms from +-inf in the archive); the tempered world
    has T = 0 at snooker and at ordinary generations;
  * every main world has steps that a wrong kernel would decide otherwise -- the Jacobian's exponent one off in either direction,
    the temperature ignored or applied to the Jacobian too, a blocked handle's quadratic form summed in one piece -- at K
    boundaries and away from them, and the edge worlds show both outcomes in their last wave (three invalid steps on three rows);
    the planned kernel names are exactly the built-in instantiations and the program units of d = 2, 3, 4, 7, 32;
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


@pytest.mark.parametrize("name", list(sc.MAIN))
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


@pytest.mark.parametrize("name", list(sc.MAIN))
def test_every_world_has_the_steps_a_wrong_kernel_decides_otherwise(oracle, name):
    """Each count is of steps on which the bit comparison would catch the named wrong kernel; three of each, this project's usual count."""
    w, _, run = sc.reference(oracle, name)
    c = sc.step_counts(oracle, w, run)
    print(name, {k: v for k, v in c.items() if not isinstance(v, set)})
    assert c["flip_lo"] >= 3 and c["flip_hi"] >= 3, f"{name}: decisions that differ with the exponent d - 2: {c['flip_lo']}, with d: {c['flip_hi']}"
    sn = sc.snooker_generations(w)
    assert any(g % w["K"] == 0 for g in sn), name
    assert c["b_acc"] >= 3 and c["b_rej"] >= 3, f"{name}: at multiples of K {c['b_acc']} accepted, {c['b_rej']} rejected"
    if any(g % w["K"] != 0 for g in sn):
        assert c["nb_acc"] >= 3 and c["nb_rej"] >= 3, f"{name}: away from multiples of K {c['nb_acc']} accepted, {c['nb_rej']} rejected"
    else:
        assert c["nb_acc"] == c["nb_rej"] == 0
    if w["temperature"] is not None:
        assert c["t_ignored"] >= 3, f"{name}: decisions that differ with T ignored: {c['t_ignored']}"
        assert c["t_jacobian"] >= 3, f"{name}: decisions that differ with the Jacobian divided by T too: {c['t_jacobian']}"
        assert {0.0, 1e-300, 1e300} <= c["T_at_snooker"], name
        if name != "mvn5_tempered":              # a plain piece with snooker and ordinary generations in it
            plain = [(a, b) for a, b, t in w["pieces"] if not t]
            assert len(plain) == 1 and any(a <= g <= b for a, b in plain for g in sn) and any(a <= g <= b and g not in sn for a, b in plain for g in range(a, b + 1))
    else:
        assert c["T_at_snooker"] == set() and all(not t for _, _, t in w["pieces"])
    if len(w["blocks"]) > 1:
        differ, accepted = sc.grouping_counts(oracle, w, run)
        if name == "mvn8_inter":
            assert differ == 0, "an interleaved structure groups nothing"
        else:
            assert accepted >= 3, f"{name}: {differ} proposals with other bits in the ungrouped order, {accepted} of them accepted"


def test_the_worlds_with_tempered_or_grouped_steps_are_the_ones_meant():
    assert {n for n, df in sc.MAIN.items() if df[4].get("tempered")} == {n for n in sc.MAIN if n.endswith("_tempered")} and \
        len([n for n in sc.MAIN if n.endswith("_tempered")]) == 11
    assert {n for n, df in sc.MAIN.items() if "blocks" in df[4]} == {"mvn6_blocks", "mvn10_halves", "mvn20_4x5", "mvn8_inter", "mvn10_halves_tempered"}
    assert list(sc.MAIN)[:16] == list(sc.WORLDS) and len(sc.MAIN) == 41 and not set(sc.MAIN) & set(sc.EDGE_WORLDS)


@pytest.mark.parametrize("name", list(sc.EDGE_WORLDS))
def test_every_edge_world_is_at_its_edge(oracle, name):
    w, ref, run = sc.reference(oracle, name)
    facts = [f for _, _, f in run.steps]
    sn = sc.snooker_generations(w)
    assert run.snooker_generations == sn and len(facts) == w["N"] * len(sn)
    assert all(f["ia"] not in (f["i1"], f["i2"]) and f["i1"] != f["i2"] for f in facts)
    assert all(w["gamma_s"][0] <= f["gamma_s"] <= w["gamma_s"][1] for f in facts)
    assert ref["M"] == w["Z0"].shape[0] + w["N"] * (w["G"] // w["K"])
    c = sc.step_counts(oracle, w, run)
    print(name, {k: v for k, v in c.items() if not isinstance(v, set)})
    if name == "mvn5_never":                     # by its definition: no snooker generation in the run
        assert sn == [] and w["every"] > w["G"]
        return
    assert sn, name
    if w["N"] >= 63:
        assert c["last_wave"] == {True, False}, f"{name}: the last wave's outcomes"
    if w["three_rows"]:
        assert w["Z0"].shape[0] == 3 and w["N"] in (1, 2)
        assert c["accepted"] >= 1 and c["rejected"] >= 1 and c["invalid"] >= 3, name
    if w["needs_invalid"]:
        assert c["invalid"] >= 3, name
    if w["gamma_s"][0] == w["gamma_s"][1]:
        assert {f["gamma_s"] for f in facts} == {w["gamma_s"][0]} and c["accepted"] >= 10 and c["rejected"] >= 10


def test_the_edge_worlds_are_invalid_in_the_ways_they_claim(oracle):
    for name in ("rosenbrock7_own_row", "mvn8_own_row", "mvn10_own_row"):
        _, _, own = sc.reference(oracle, name)
        assert sum(f["e2"] == 0.0 for _, _, f in own.steps) >= 3, name
    for name in ("mvn8_inf", "mvn10_inf"):
        _, ref, inf = sc.reference(oracle, name)
        assert any(math.isinf(f["e2"]) for _, _, f in inf.steps) and any(math.isnan(v) or math.isinf(v) for v in (f.get("f2", 1.0) for _, _, f in inf.steps)), name
        assert np.isfinite(ref["chain"][:, :, [g - 1 for g in inf.snooker_generations]]).all(), name


@pytest.mark.parametrize("name,E", sc.LAGGED)
def test_the_lagged_worlds_accept_steps_at_their_boundaries(oracle, name, E):
    """A kernel that stored the state from before the step as the boundary snapshot would be wrong in every accepted step of a
    snooker generation that is a multiple of K; the lag shows inside the run, not only in the final archive."""
    w, ref, run = sc.lagged_reference(oracle, name, E)
    assert w["temperature"] is None and w["closure"] is None
    c = sc.step_counts(oracle, w, run)
    assert c["b_acc"] >= 3 and c["b_rej"] >= 3, (name, c["b_acc"], c["b_rej"])
    _, plain, _ = sc.reference(oracle, name)
    first_seen = (-(-1 // E) * E + E) * w["K"] + 1
    assert first_seen <= w["G"] and ref["M"] == plain["M"] and ref["Z"].shape == plain["Z"].shape
    assert np.array_equal(ref["chain"][:, :, :w["K"]], plain["chain"][:, :, :w["K"]]) and not np.array_equal(ref["chain"], plain["chain"])
    assert not np.array_equal(ref["Z"], plain["Z"])


def test_the_planned_kernel_names_are_every_instantiation(oracle):
    """The ten specialised built-in instantiations, the three run-time-d ones and the program units of d = 2, 3, 4, 7 and 32: a world
    dropped later is noticed here."""
    assert len(sc.PLANNED_NAMES) == 10 + 3 + 5
    assert {sc.planned_kernel(sc.world(n)) for n in sc.MAIN} == sc.PLANNED_NAMES
    assert {sc.planned_kernel(sc.world(n)) for n in sc.MAIN if n.endswith("_tempered")} == {
        "demcz::snooker_kernel<MVNORMAL, 5>", "demcz::snooker_kernel<MVNORMAL, 8>", "demcz::snooker_kernel<MVNORMAL, 10>",
        "demcz::snooker_kernel<MVNORMAL, 20>", "demcz::snooker_kernel_generic<MVNORMAL>", "demcz::snooker_kernel<ISO_QUAD, 10>",
        "demcz::snooker_kernel_generic<ISO_QUAD>", "demcz::snooker_kernel<LINREG_SSE, 10>", "demcz::snooker_kernel<LINREG_SSE, 26>",
        "demcz::snooker_kernel_generic<LINREG_SSE>", "demcz::snooker_kernel<4, 7> (program)"}


def test_the_schedules_end_calls_on_and_in_front_of_snooker_generations():
    for name in sc.ALL:
        w = sc.world(name)
        sn, ends = set(sc.snooker_generations(w)), [b for _, b, _ in w["pieces"]]
        assert [a for a, _, _ in w["pieces"]] == [1] + [b + 1 for b in ends[:-1]] and ends[-1] == w["G"], name
        if sn:
            assert any(b in sn for b in ends) and any(b + 1 in sn and b not in sn or (w["every"] == 1 and b + 1 in sn) for b in ends), name
        counts = sc.launches_after(w)
        assert counts == sorted(counts) and counts[-1] >= len(sn) + (0 if w["every"] == 1 else 1), name
    # the rule by hand: K = 10, every = 3, calls that end at 2, 3, 20, 30, 40
    # 1-2 | 3 | 4-5 6 7-8 9 10 11 12 13-14 15 16-17 18 19-20 | 21 22-23 24 25-26 27 28-29 30 | 31-32 33 34-35 36 37-38 39 40
    assert sc.launches_after(sc.world("mvn7")) == [1, 2, 14, 21, 28]
    assert sc.launches_after(sc.world("mvn5_never")) == [1, 3, 5] and sc.launches_after(sc.world("mvn5_k1")) == [1, 2, 20, 31, 40]


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
