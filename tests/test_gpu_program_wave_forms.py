"""GPU: program targets on the wave-per-chain layout in every dimension, every form and every pass outcome, bit for bit against a
reference that is not another layout of the library.

A handle created with lanes_per_chain = DEMCZ_LAYOUT_PROGRAM_WAVE runs a hipRTC unit of its own (demcz_program.hip, UNIT_WAVE),
compiled per d: the general window_kernel_ps (d = 2..5) / window_kernel_pw (d = 6..32) in four instantiations LIVE x TEMPER, the
candidate adds reading their increments from LDS at every d >= 6, the user's function called EXEC-masked on lanes 1..31, a full
drain of the vector-memory queue in place of the counted waits.  tests/program_wave_cases.py holds the worlds: MvNormal restated as
a program at every d = 2..32 and the isotropic quadratic at five dimensions against the oracle's built-in targets, Rosenbrock at
four against the oracle's loop around its Python twin; one handle per world whose schedule reaches the four forms and passes of
every length inside and outside LIVE launches -- in which, by the reference alone (tests/test_program_wave_cases.py), every accept
/ reject outcome of every pass length occurs and every tempered call depends on its temperatures.  After every call the kernel's
name, the LIVE status, the count of window launches and the layout are held to the plan; at the end chain, log_obj, X, logp, Z
(helpers.same_bits), M, the per-generation changed counts and the ballots' changed_total.  Every case compiles its own program.
No tolerance anywhere."""
import numpy as np
import pytest

import program_wave_cases as pc
from demc_jl_amd import _lib
from helpers import same_bits

pytestmark = pytest.mark.gpu

WAVE = _lib.LAYOUT_PROGRAM_WAVE


def engine_run(demc, case):
    """The library over the case's pieces on one handle: the reference's dict, with `changed` from generation `counted_from` on,
    `totals` {first generation: (changed_total, from the ballots)}, and `names`, `launches`, `live`, `layout` after every piece."""
    w, N, d, G, K = case["problem"], case["N"], case["d"], case["G"], case["K"]
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G if case["history"] else 0, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=case["seed"], target=case["program"](), lanes_per_chain=WAVE)
    try:
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        names, launches, live, layout = [], [], [], []
        for a, b, tempered, _ in case["pieces"]:
            e.run(a, b, case["gamma"], case["temperature"][a - 1:b] if tempered else None)
            names.append(e.kernel_name())
            launches.append(e.info()["window_launches"])
            live.append(tuple(e.live_status()))
            layout.append(e.info()["lanes_per_chain"])
            if b == case["resume_at"]:
                X, lp, Z, M = e.get_state()
                e.set_state(np.array(X), np.array(lp), np.array(Z[:M]))
        counted_from = 1 if case["resume_at"] is None else case["resume_at"] + 1
        chain, lobj = e.get_history(1, G) if case["history"] else (None, None)
        changed = e.get_changed(counted_from, G) if case["history"] else None
        X, lp, Z, M = e.get_state()
        # from generation 1 (behind a hand-back: from the generation behind it), and from every launch's first generation and the
        # generation behind that: whole launches, and whole launches less their first generation's own count
        firsts = sorted({counted_from} | {g for l in pc.launch_pieces(case) for g in (l[0], l[0] + 1) if counted_from <= g <= G})
        totals = {g: e.changed_total(g, G, with_source=True) for g in firsts}
        return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=changed,
                    counted_from=counted_from, totals=totals, names=names, launches=launches, live=live, layout=layout)
    finally:
        e.close()


def _run(demc, oracle, case):
    """One world: the plan held after every piece, the results against the reference."""
    what = case["name"]
    got = engine_run(demc, case)
    d, K = case["d"], case["K"]
    assert got["layout"] == [WAVE] * len(case["pieces"]), what
    launches = pc.launch_pieces(case)
    for (a, b, _, _), name, status in zip(case["pieces"], got["names"], got["live"]):
        form = [l for l in launches if l[1] <= b][-1][3]                      # (the name read behind a piece is its last launch's)
        assert name == pc.kernel_name(d, form), f"{what}, generations {a}..{b}: planned {form} ({pc.kernel_name(d, form)}), ran {name}"
        assert status == (case["live"], 0), \
            f"{what}, generations {a}..{b}: LIVE status {status} (a LIVE launch that timed out and was redone did not produce these numbers)"
    assert got["launches"] == pc.launches_after(case), f"{what}: window launches behind every piece"
    ref = pc.reference_run(oracle, case)
    same_bits(got, ref, keys=("chain", "log_obj", "X", "logp", "Z") if case["history"] else ("X", "logp", "Z"), what=what)
    assert got["M"] == ref["M"], what
    c0 = got["counted_from"]
    if case["history"]:
        assert np.array_equal(got["changed"], ref["changed"][c0 - 1:]), f"{what}: the per-generation counts from generation {c0} on"
    starts = {l[0] for l in launches}
    for g, (total, from_ballots) in got["totals"].items():
        assert total == int(ref["changed"][g - 1:].sum()), f"{what}: changed_total from generation {g}: {total} (from the ballots: {from_ballots})"
        # (demcz_get_changed_total: the ballots answer for whole launches, with or without the first one's first generation)
        assert from_ballots == (g in starts or g - 1 in starts), f"{what}: changed_total from generation {g}: from the ballots: {from_ballots}"
        assert from_ballots, what
    assert {c0, c0 + 1} <= set(got["totals"]) and len(got["totals"]) >= min(2 * len(launches), 3)
    return got


# ---- every dimension, every form, every outcome --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", pc.MAIN_WORLDS, ids=["%s-%d" % w for w in pc.MAIN_WORLDS])
def test_every_dimension_every_form(demc, oracle, kind, d):
    case = pc.main_case(kind, d)
    assert {p[3] for p in case["pieces"]} == set(pc.FORMS)
    got = _run(demc, oracle, case)
    assert set(got["names"]) == {pc.kernel_name(d, f) for f in pc.FORMS} and got["launches"][-1] == len(case["pieces"])


# ---- named edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N", pc.TINY)
def test_tiny_and_ragged_populations(demc, oracle, d, N):
    """Idle chain waves in a four-chain workgroup, a ragged last one."""
    _run(demc, oracle, pc.tiny_case(d, N))


def test_the_largest_population_runs_one_launch_per_window(demc, oracle):
    case = pc.largest_case()
    got = _run(demc, oracle, case)
    assert got["launches"] == [2, 4] and set(got["live"]) == {(False, 0)}
    assert all(", false," in n for n in got["names"]), got["names"]


@pytest.mark.parametrize("k", list(pc.OTHER_K))
@pytest.mark.parametrize("d", pc.OTHER_K_DIMS)
def test_other_window_lengths_on_live_launches(demc, oracle, d, k):
    """K = 1: every pass is one generation; 3 and 4: passes of K; 7 and 12: full passes and passes of two."""
    got = _run(demc, oracle, pc.other_k_case(d, k))
    assert got["launches"] == [1, 2] and all(", true," in n for n in got["names"])


@pytest.mark.parametrize("d", pc.CUT_DIMS)
def test_a_cut_tempered_call_starts_a_launch_at_an_odd_temperature(demc, oracle, d):
    import small_wave_cases as sw
    got = _run(demc, oracle, pc.cut_case(d))
    assert got["launches"] == sw.CUT_LAUNCHES, "the tempered call was not cut behind its fifteenth generation"


@pytest.mark.parametrize("d", pc.EDGE_TEMPERATURE_DIMS)
def test_zero_tiny_and_huge_temperatures(demc, oracle, d):
    case = pc.edge_temperature_case(d)
    assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist())
    assert _run(demc, oracle, case)["launches"] == [1]


@pytest.mark.parametrize("d", pc.NO_HISTORY_DIMS)
def test_no_history_kept(demc, oracle, d):
    """Gcap = 0: state, archive and the ballots' changed_total."""
    got = _run(demc, oracle, pc.no_history_case(d))
    assert got["chain"] is None and got["launches"] == [1] and all(src for _, src in got["totals"].values())


@pytest.mark.parametrize("d", pc.RESUMED_DIMS)
def test_a_run_carried_on_after_set_state(demc, oracle, d):
    """demcz_set_state in the middle of a window: what was prepared is discarded, the handle's parameters and counters carry on;
    changed_total is asked from the generation behind the hand-back."""
    case = pc.resumed_case(d)
    got = _run(demc, oracle, case)
    assert got["counted_from"] == pc.RESUME_AT + 1 and min(got["totals"]) == pc.RESUME_AT + 1
    assert got["launches"] == list(range(1, len(case["pieces"]) + 1))
