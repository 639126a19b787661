"""CPU tier of the crossover generation: the worlds of tests/crossover_cases.py are worth running, and the proposal samples the
right distribution -- from the reference alone (tests/crossover_reference.py).

  * every world with ncr = 3, delta_max = 3 has at least 10 accepted and 10 rejected steps in each of the nine (class, delta)
    cells; worlds with d <= 5 have at least 10 fallback steps, accepted and rejected ones among them; every tempered world has
    at least 10 steps that the untempered comparison decides otherwise; the per-class tried counts add up to chains x crossover
    generations; the worlds with weights of zero never draw those classes;
  * the planned kernel names are exactly the built-in instantiations and the program units of d = 2, 3, 4, 7, 32;
  * a run cut into pieces is the run in one piece; a resumed run follows the streams; snooker generations replace crossover
    generations at the multiples of `every` and read the same stride;
  * the drivers refuse, before they build an engine, what the library would;
  * the moment test: the proposal as the only move on a correlated six-parameter Gaussian recovers every mean and variance within
    four of the runs' own standard errors."""
import numpy as np
import pytest

import crossover_cases as cc
import crossover_reference as cr
from helpers import same_bits


@pytest.mark.parametrize("name", list(cc.ALL))
def test_every_world_meets_its_conditions(oracle, name):
    w, ref, run = cc.reference(oracle, name)
    n_cr = len(run.crossover_generations)
    assert n_cr == sum(1 for g in range(1, w["G"] + 1) if not (w["every"] and g % w["every"] == 0))
    tried, accepted = run.counts()
    assert tried.sum() == w["N"] * n_cr == len(run.steps) and (accepted <= tried).all()
    assert len(run.snooker_steps) == w["N"] * (w["G"] - n_cr)
    assert ref["M"] == w["Z0"].shape[0] + w["N"] * (w["G"] // w["K"])
    cells = cc.cell_counts(run)
    print(name, {k: tuple(v) for k, v in sorted(cells.items())}, "fallback", cc.fallback_counts(run))
    if (w["ncr"], w["delta_max"]) == (3, 3) and w["weights"] is None:
        assert set(cells) == {(m, dl) for m in range(3) for dl in (1, 2, 3)}, name
        assert all(a >= 10 and r >= 10 for a, r in cells.values()), (name, cells)
    if w["weights"] is not None:
        assert all(tried[k] == 0 for k, wk in enumerate(w["weights"]) if wk == 0) and all(tried[k] > 0 for k, wk in enumerate(w["weights"]) if wk > 0)
    if w["d"] <= 5 and w["N"] >= 64 and w["ncr"] >= 2:          # (one class selects everything: no fallback)
        fa, fr = cc.fallback_counts(run)
        assert fa >= 10 and fr >= 10, (name, fa, fr)
    if w["temperature"] is not None:
        assert cc.tempered_flips(run) >= 10, name
        assert {0.0, 1e-300, 1e300} <= {f["T"] for _, _, f in run.steps}
    # the mask: never empty, inside d, the fallback exactly where nothing was selected, unselected parameters bit for bit
    for _, _, f in run.steps:
        assert 0 < f["mask"] < (1 << w["d"]) and 1 <= f["delta"] <= w["delta_max"] and 0 <= f["m"] < w["ncr"]
        assert not f["fallback"] or f["mask"] == 1 << f["pstar"]
    if w["d"] > 32:
        assert any(f["mask"] >> 32 for _, _, f in run.steps)
    if w["d"] == 64:
        assert any(f["mask"] >> 63 & 1 and f["accepted"] for _, _, f in run.steps) and any(not f["mask"] >> 63 & 1 and f["accepted"] for _, _, f in run.steps)


def test_the_small_worlds_are_at_their_edges(oracle):
    w, ref, run = cc.reference(oracle, "mvn5_two_rows_k1")
    assert w["Z0"].shape[0] == 2 and w["K"] == 1 and w["N"] == 2
    first = [f for g, _, f in run.steps if g == 1]
    assert all(set(p) == {0, 1} for f in first for p in f["pairs"])            # two rows: every pair is both of them
    assert {f["accepted"] for _, _, f in run.steps} == {True, False}
    w, _, run = cc.reference(oracle, "mvn5_n1")
    assert w["N"] == 1 and {f["accepted"] for _, _, f in run.steps} == {True, False}
    w, _, run = cc.reference(oracle, "mvn7_n64")
    assert w["N"] == 64 and {f["accepted"] for _, c, f in run.steps if c == 63} == {True, False}
    w, ref, run = cc.reference(oracle, "box4")
    assert np.isinf(w["Z0"]).sum() == 3 and np.isfinite(ref["chain"]).all()
    assert sum(f["lp_prop"] == -np.inf for _, _, f in run.steps) >= 10 and sum(not np.isfinite(f["xp"]).all() for _, _, f in run.steps) >= 10
    # both outcomes in the part-filled wave of every main world
    for name in cc.ALL:
        w, _, run = cc.reference(oracle, name)
        if w["N"] == cc.N:
            assert {f["accepted"] for _, c, f in run.steps if c >= 64} == {True, False}, name


def test_the_planned_kernel_names_are_every_instantiation():
    """The ten specialised built-in instantiations, the three run-time-d ones and the program units of d = 2, 3, 4, 7 and 32: a
    world dropped later is noticed here."""
    assert len(cc.PLANNED_NAMES) == 10 + 3 + 5
    assert {cc.planned_kernel(cc.world(n)) for n in cc.ALL} == cc.PLANNED_NAMES
    tempered = {cc.planned_kernel(cc.world(n)) for n in cc.ALL if cc.ALL[n][3].get("tempered")}
    assert tempered == {"demcz::window_kernel_cr<MVNORMAL, 5>", "demcz::window_kernel_cr<MVNORMAL, 20>", "demcz::window_kernel_cr_generic<MVNORMAL>",
                        "demcz::window_kernel_cr<ISO_QUAD, 10>", "demcz::window_kernel_cr_generic<ISO_QUAD>", "demcz::window_kernel_cr<LINREG_SSE, 10>",
                        "demcz::window_kernel_cr_generic<LINREG_SSE>", "demcz::window_kernel_cr<4, 7> (program)"}
    assert {cc.world(n)["d"] for n in cc.ALL if cc.planned_kernel(cc.world(n)).startswith("demcz::window_kernel_cr_generic")} >= {4, 7, 9, 33, 64}


def test_a_reference_run_in_pieces_is_the_run_in_one(oracle):
    for name in ("mvn7_snooker", "rosenbrock7", "mvn5_tempered"):
        w, ref, _ = cc.reference(oracle, name)
        run = cc.crossover_run(oracle, w)
        a = 1
        for b in cc.uneven_cuts(w):
            run.run(a, b, w["gamma"], None if w["temperature"] is None else w["temperature"][a - 1:b])
            a = b + 1
        same_bits(run.result(), ref, what=name)


def test_a_resumed_reference_follows_the_streams(oracle):
    """rng_offset = 20 with snooker every 4 on a 15-generation first part: the second part's choices are those of the whole run."""
    w, ref, whole = cc.reference(oracle, "mvn7_snooker")
    first = cc.crossover_run(oracle, w)
    first.run(1, 15, w["gamma"])
    r1 = first.result()
    second = cc.crossover_run(oracle, w, Z0=r1["Z"], X0=r1["X"], lp0=r1["logp"], rng_offset=15, G=25)
    second.run(1, 25, w["gamma"])
    assert [g + 15 for g in second.snooker_generations] == [g for g in whole.snooker_generations if g > 15]
    r2 = second.result()
    assert np.array_equal(r2["chain"], ref["chain"][:, :, 15:]) and np.array_equal(r2["Z"], ref["Z"])
    assert [f["mask"] for _, _, f in second.steps] == [f["mask"] for g, _, f in whole.steps if g > 15]


def test_snooker_generations_replace_crossover_generations(oracle):
    w, ref, run = cc.reference(oracle, "mvn5_snooker")
    assert run.snooker_generations == [g for g in range(1, w["G"] + 1) if g % 4 == 0] and run.S == cr.stride(5, 3) == 10
    assert sum(f["accepted"] for _, _, f in run.snooker_steps) >= 10 and sum(f["valid"] and not f["accepted"] for _, _, f in run.snooker_steps) >= 10
    plain = cc.crossover_run(oracle, w, every=0)
    plain.run(1, w["G"], w["gamma"])
    p = plain.result()
    assert np.array_equal(p["chain"][:, :, :3], ref["chain"][:, :, :3]) and not np.array_equal(p["chain"][:, :, 3], ref["chain"][:, :, 3])
    # a K boundary that is a snooker generation (20, 40) and ones that are not
    assert {g for g in run.snooker_generations if g % w["K"] == 0} == {20, 40}


def test_the_drivers_refuse_before_they_build_an_engine(demc):
    from oracle_engine import OracleEngine
    w = demc.workloads.mvnormal_problem(5, 8)
    args = (w["Zinit"], 8, 10, 20)
    tail = (w["eps_scale"], w["gamma"])
    for driver in (demc.demcz_sample, demc.demcz_anneal):
        with pytest.raises(ValueError, match="one-lane"):
            driver(w["target"], *args, 1, [range(5)], *tail, verbose=False, crossover=(3, 3), lanes_per_chain=16)
        with pytest.raises(ValueError, match="device target"):
            driver(lambda x: -float(np.sum(x * x)), *args, 1, [range(5)], *tail, verbose=False, crossover=(3, 3))
        with pytest.raises(ValueError, match="one block"):
            driver(w["target"], *args, 2, [range(2), range(2, 5)], *tail, verbose=False, crossover=(3, 3))
        with pytest.raises(ValueError, match="set_crossover"):
            driver(w["target"], *args, 1, [range(5)], *tail, verbose=False, crossover=(3, 3), engine_factory=OracleEngine)
        for bad in ((9, 3), (3, 0), (3, 4), (-1, 1), (3,)):
            with pytest.raises(ValueError, match="crossover"):
                driver(w["target"], *args, 1, [range(5)], *tail, verbose=False, crossover=bad)
    # crossover = None and ncr = 0 leave the drivers as they were: the oracle-backed engine runs
    for off in (None, (0, 1)):
        mc, _ = demc.demcz_sample(w["target"], *args, 1, [range(5)], *tail, verbose=False, crossover=off, engine_factory=OracleEngine)
        assert mc.chain.shape == (8, 5, 20)
    assert len(demc.DEMCopt.__dataclass_fields__) == 14


def test_the_library_exports_the_two_entry_points(demc):
    L = demc._lib
    assert {"demcz_set_crossover", "demcz_get_crossover"} <= set(L.SYMBOLS)
    lib = L.load()
    assert lib.demcz_set_crossover and lib.demcz_get_crossover
    assert any(p.name == "demcz_crossover_inst.hip" for p in L.sources())


def test_check_compiles_the_crossover_kernel_of_a_program(demc):
    """check() builds the unit the handle will load, the crossover kernel included, without a device.  A program that defines a
    name the crossover kernel's own text uses compiles for no kernel of the unit and fails at check() with the compiler's log."""
    from program_texts import ROSENBROCK
    demc.ProgramTarget(ROSENBROCK, 7).check()
    bad = demc.ProgramTarget("#define cr_selects 0\n" + ROSENBROCK, 7)
    with pytest.raises(demc.DemczError) as ei:
        bad.check()
    assert "demcz_kernels_crossover.h" in str(ei.value)


# ---- the moment test -------------------------------------------------------------------------------------------------------------------
D, CHAINS, GENS, KM, RUNS = 6, 64, 3000, 10, 16


def _moments(seed):
    """The crossover proposal (3, 3) as the only move: 64 chains, 3000 generations, an archive started at 10 d over-dispersed rows
    that takes the population every K-th generation; mean and variance per parameter over the second half."""
    rng = np.random.default_rng(seed)
    idx = np.arange(D)
    Sigma = 0.7 ** np.abs(idx[:, None] - idx[None, :])
    mu = np.linspace(-1.0, 1.0, D)
    P = np.linalg.inv(Sigma)
    logp = lambda X: -0.5 * np.einsum("ni,ij,nj->n", X - mu, P, X - mu)
    L = np.linalg.cholesky(Sigma)
    Z = np.empty((10 * D + CHAINS * (GENS // KM), D))
    M = 10 * D
    Z[:M] = mu + 2.0 * rng.standard_normal((M, D)) @ L.T
    X = mu + 2.0 * rng.standard_normal((CHAINS, D)) @ L.T
    lp = logp(X)
    kept = np.empty((GENS // 2, CHAINS, D))
    for g in range(1, GENS + 1):
        X, lp, _, _ = cr.crossover_population_step(rng, X, lp, Z[:M], logp, 2.38, 1e-4, 3, 3)
        if g > GENS // 2:
            kept[g - GENS // 2 - 1] = X
        if g % KM == 0:
            Z[M:M + CHAINS] = X
            M += CHAINS
    flat = kept.reshape(-1, D)
    return np.concatenate([flat.mean(axis=0) - mu, flat.var(axis=0, ddof=1) - np.diag(Sigma)])


def test_the_proposal_samples_the_target():
    err = np.array([_moments(20090301 + s) for s in range(RUNS)])          # (runs, 2 D): mean and variance errors
    se = err.std(axis=0, ddof=1) / np.sqrt(RUNS)
    z = err.mean(axis=0) / se
    print("z of the means", np.round(z[:D], 2), "of the variances", np.round(z[D:], 2), "standard errors", np.round(se, 4))
    assert (np.abs(z) <= 4.0).all(), z
