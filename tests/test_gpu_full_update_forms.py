"""GPU: every full-update lane, matrix and one-lane kernel in every form, bit for bit against the oracle.

tests/full_update_cases.py holds the worlds: per kernel one handle whose schedule of demcz_run calls reaches every form -- split
layout: LIVE / non-LIVE x plain / tempered; fused and one lane per chain: plain / tempered, calls cut inside a window and across
boundaries -- and in which, by the oracle alone (tests/test_full_update_cases.py), a chain moves in about half of its generations,
every (previous outcome, this outcome) pair occurs in every form and every tempered piece depends on its temperatures.  After
every piece the kernel's reported name, the LIVE status and the count of window launches are held to the plan: the 13 full-update
instantiations of window_kernel_ml, the three of window_kernel_lr16 and the two of window_kernel_lr8s, window_kernel<T, d, true>
for every specialised (T, d) and the generic kernel for three targets; four-wave workgroups on 8 and 16 lanes; the observation
counts at which the matrix kernels' tiling and their LDS-fit rules turn.  At the end chain, log_obj, X, logp, Z, then M, then the
ballots' changed_total from generation 1 and from the last launch's first generation are compared.  No tolerance anywhere
(DESIGN.md section 3)."""
import pytest

import full_update_cases as fc
from block_cases import oracle_run
from helpers import SPLIT
from test_gpu_block_forms import _device_cus, _same_as_oracle, engine_run

pytestmark = pytest.mark.gpu


def _run(demc, oracle, monkeypatch, case, layout, env=(), live=True, history=True, resume_at=None):
    """One world on one handle, held to full_update_cases.plan.  live = None: a split handle that the device may or may not hold in
    one LIVE launch -- its LIVE status decides which plan it is held to."""
    for v in env:
        monkeypatch.setenv(v, "1")                      # (read in demcz_create)
    lanes = {"fused": fc.lanes_of(case) if layout == "fused" else 0, "split": SPLIT, "one": 1}[layout]
    changed_from = resume_at + 1 if resume_at else 1    # (demcz_set_state opens the history window anew)
    got = engine_run(demc, case, lanes, history=history, resume_at=resume_at, changed_from=changed_from,
                     tail_from=lambda went_live: fc.last_launch_from(case, layout, went_live))
    what = f"{case['name']}, {layout}{' ' + ' '.join(env) if env else ''}"
    went_live = layout == "split" and (got["live"][0][0] if live is None else live)
    plan = fc.plan(case, layout, env, live=went_live, cold_behind=(resume_at,) if resume_at else ())
    assert got["layout"] == lanes, what
    assert len(got["names"]) == len(plan) == len(case["pieces"])
    for (a, b, _, form), (name, _), ran, status in zip(case["pieces"], plan, got["names"], got["live"]):
        assert ran == name, f"{what}, generations {a}..{b} ({form}): planned {name}, ran {ran}"
        assert status == ((True, 0) if went_live else (False, 0)), \
            f"{what}, generations {a}..{b}: LIVE status {status} (a LIVE launch that timed out and was redone did not produce these numbers)"
    assert got["launches"] == [c for _, c in plan], f"{what}: window launches behind every piece"
    ref = oracle_run(oracle, case)
    _same_as_oracle(got, ref, what, keys=("chain", "log_obj", "X", "logp", "Z") if history else ("X", "logp", "Z"), changed_from=changed_from)
    g = fc.last_launch_from(case, layout, went_live)
    assert got["changed_tail"] == int(ref["changed"][g - 1:].sum()), \
        f"{what}: changed_total from generation {g}: {got['changed_tail']} (from the ballots: {got['tail_from_ballots']})"
    got["went_live"] = went_live
    return got


# ---- A: window_kernel_ml ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", fc.FUSED_WORLDS)
def test_fused_lane_kernels_every_form(demc, oracle, monkeypatch, world):
    got = _run(demc, oracle, monkeypatch, fc.case_of(world), "fused")
    assert len(set(got["names"])) == 1 and "window_kernel_ml<" in got["names"][0]


@pytest.mark.parametrize("world", fc.SPLIT_WORLDS)
def test_split_lane_kernel_every_form(demc, oracle, monkeypatch, world):
    case = fc.case_of(world)
    got = _run(demc, oracle, monkeypatch, case, "split")
    assert {(p[3], n) for p, n in zip(case["pieces"], got["names"])} == \
        {(f, "demcz::window_kernel_ml<MVNORMAL, 20, 16, true, %s>" % ("true" if f.startswith("LIVE") else "false")) for f in fc.FORMS}


def _four_wave(demc, oracle, monkeypatch, world, sign, layout, live):
    """Nothing the library reports exposes the workgroup shape: this asserts the inequality demcz_create decides it by -- chain
    waves >= 4 x the device's CUs -- and relies on it.  The last workgroup is partly filled."""
    cus = _device_cus()
    case = fc.four_wave_case(world, sign, cus)
    per_wave = 64 // fc.lanes_of(case)
    assert fc.chain_waves(case) >= 4 * cus and case["N"] % (4 * per_wave) != 0
    got = _run(demc, oracle, monkeypatch, case, layout, live=live)
    print(case["name"], "N", case["N"], "CUs", cus, layout, "LIVE" if got["went_live"] else "one launch per K-window")


@pytest.mark.parametrize("world", fc.FOUR_WAVE_FUSED)
def test_four_wave_workgroups_fused(demc, oracle, monkeypatch, world):
    _four_wave(demc, oracle, monkeypatch, world, 1, "fused", True)


@pytest.mark.parametrize("world,sign", fc.FOUR_WAVE_SPLIT, ids=["%s-%s" % (w, "over" if s > 0 else "under") for w, s in fc.FOUR_WAVE_SPLIT])
def test_four_wave_workgroups_split(demc, oracle, monkeypatch, world, sign):
    """One workgroup more than the device has CUs ("over") or one per CU ("under"): LIVE where the device holds them together,
    otherwise one launch per K-window, by the handle's own LIVE status."""
    _four_wave(demc, oracle, monkeypatch, world, sign, "split", None)


@pytest.mark.parametrize("world,N,layout", fc.TINY)
def test_tiny_populations(demc, oracle, monkeypatch, world, N, layout):
    """Idle chain groups in the only wave."""
    _run(demc, oracle, monkeypatch, fc.edge_case(world, N), layout)


@pytest.mark.parametrize("world,layout", fc.NO_HISTORY)
def test_no_history_kept(demc, oracle, monkeypatch, world, layout):
    """Gcap = 0: state, archive and the ballots' changed_total."""
    got = _run(demc, oracle, monkeypatch, fc.edge_case(world), layout, history=False)
    assert got["from_ballots"] and got["tail_from_ballots"]


@pytest.mark.parametrize("world,layout", fc.ZERO_TEMPERATURE)
def test_zero_tiny_and_huge_temperatures(demc, oracle, monkeypatch, world, layout):
    case = fc.zero_temperature_case(world)
    assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist())
    _run(demc, oracle, monkeypatch, case, layout)


@pytest.mark.parametrize("world,layout", fc.RESUMED)
def test_a_run_carried_on_after_set_state(demc, oracle, monkeypatch, world, layout):
    _run(demc, oracle, monkeypatch, fc.resumed_case(world), layout, resume_at=fc.RESUME_AT)


# ---- B: the d = 10 regression matrix kernels ----------------------------------------------------------------------------------------------
_LR = pytest.mark.parametrize("layout,env", fc.LR_HANDLES, ids=fc.LR_HANDLE_IDS)


@_LR
def test_regression_matrix_kernels_every_form(demc, oracle, monkeypatch, layout, env):
    case = fc.case_of(fc.LR_WORLD)
    got = _run(demc, oracle, monkeypatch, case, layout, env)
    want = {"lr16": 1, "lr8s": 2, "lr16_split": 2}[fc.LR_HANDLE_IDS[fc.LR_HANDLES.index((layout, env))]]
    assert len(set(got["names"])) == want, got["names"]


@_LR
@pytest.mark.parametrize("nobs", fc.NOBS_COUNTS)
def test_regression_observation_counts(demc, oracle, monkeypatch, nobs, layout, env):
    """The tiling's edges: ngrp = ceil(nobs / 64), the padded rows of the A operand, y_l."""
    _run(demc, oracle, monkeypatch, fc.lr_case(nobs), layout, env)


@pytest.mark.parametrize("nobs,layout,env", fc.LR_LIMITS, ids=["%d-%s" % (n, lay) for n, lay, _ in fc.LR_LIMITS])
def test_regression_lds_limits(demc, oracle, monkeypatch, nobs, layout, env):
    """The last count that fits window_kernel_lr8s (1152: 162 192 bytes of 163 840) and the first that does not (a plain split
    handle then runs window_kernel_lr16<10, true, ...>); the last that fits window_kernel_lr16 (1472: 159 504 bytes), fused and
    split, and the first that does not, which sixteen lanes run on window_kernel_ml's helper-wave form."""
    case = fc.lr_case(nobs)
    got = _run(demc, oracle, monkeypatch, case, layout, env)
    kernel = {(1152, "split"): "lr8s<10", (1153, "split"): "lr16<10, true", (1472, "split"): "lr16<10, true", (1472, "fused"): "lr16<10, false, false>",
              (1473, "fused"): "window_kernel_ml<LINREG_SSE, 10, 16"}[nobs, layout]
    assert all(kernel in n for n in got["names"]), got["names"]


def test_more_observations_than_fit_are_refused_on_the_split_layout(demc):
    case = fc.lr_case(fc.LR16_MAX_OBS + 1)
    w = case["problem"]
    with pytest.raises(demc.DemczError, match="the split layout is not built for this target / d / block structure"):
        demc.HipEngine(N=case["N"], d=10, K=case["K"], Mcap=w["Zinit"].shape[0] + case["N"] * (case["G"] // case["K"] + 1), Gcap=case["G"],
                       blockindex=case["blocks"], eps_scale=w["eps_scale"], seed=case["seed"], target=w["target"], lanes_per_chain=SPLIT).close()


@_LR
@pytest.mark.parametrize("N", fc.LR_POPULATIONS)
def test_regression_populations(demc, oracle, monkeypatch, N, layout, env):
    """Idle columns of the matrix instruction shadow chain N - 1, at sixteen and at eight chains per workgroup."""
    _run(demc, oracle, monkeypatch, fc.lr_case(N=N), layout, env)


# ---- C: one lane per chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", fc.ONE_LANE_WORLDS)
def test_one_lane_kernels_every_target(demc, oracle, monkeypatch, world):
    got = _run(demc, oracle, monkeypatch, fc.case_of(world), "one")
    assert len(set(got["names"])) == 1 and got["names"][0].endswith(", true>")


@pytest.mark.parametrize("world,N", fc.ONE_LANE_POPULATIONS)
def test_one_lane_populations(demc, oracle, monkeypatch, world, N):
    """WINDOW_BS = 64 chains a workgroup: one chain, one short of a workgroup, a full one, one more, two and one."""
    _run(demc, oracle, monkeypatch, fc.edge_case(world, N), "one")
