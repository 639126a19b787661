"""GPU: every block-update kernel in every form, bit for bit against the oracle.

tests/block_cases.py holds the worlds: per kernel and block structure one handle whose schedule of demcz_run calls reaches every
form -- split layout: LIVE / non-LIVE x plain / tempered; fused and one lane per chain: plain / tempered, calls cut inside a
window and across boundaries -- and in which, by the oracle alone (tests/test_block_cases.py), every accept / reject outcome vector
of a generation's block-steps occurs in every form and every tempered piece depends on its temperatures.  After every piece the
kernel's reported name and the LIVE status are held to the plan: all 31 instantiations of window_kernel_mlb (the reported name
leaves out the group-start-mask argument: the world's block structure decides it, block_cases.grouped), the ten one-lane block
specialisations, the generic kernel for three targets, a program's window_blocks; four-wave workgroups of the split layout at 8
and 16 lanes.  At the end chain, log_obj, X, logp, Z, M and the ballots' changed_total are compared.  No tolerance anywhere
(DESIGN.md section 3)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import block_cases as bc
from helpers import SPLIT, same_bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
L32 = "DEMCZ_MLB_L32"


def engine_run(demc, case, lanes, history=True, resume_at=None, changed_from=1, tail_from=None):
    """The library over the case's pieces on one handle: block_cases.oracle_run's dict (changed: the total), `names`, `launches`
    and `live` after every piece, `layout`.  resume_at: behind the piece that ends there the handle is given its own state back.
    changed_from: the first generation of the changed_total asked for.  tail_from: a function of the handle's LIVE status that
    gives the first generation of a second total (`changed_tail`: tests/test_gpu_full_update_forms.py, the last launch's)."""
    w, N, d, G = case["problem"], case["N"], case["d"], case["G"]
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=case["K"], Mcap=M0 + N * (G // case["K"] + 1), Gcap=G if history else 0, blockindex=case["blocks"],
                       eps_scale=w["eps_scale"], seed=case["seed"], target=w["target"], lanes_per_chain=lanes)
    try:
        layout = e.info()["lanes_per_chain"]
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        names, launches, live = [], [], []
        for a, b, tempered, _ in case["pieces"]:
            e.run(a, b, case["gamma"], case["temperature"][a - 1:b] if tempered else None)
            names.append(e.kernel_name())
            launches.append(e.info()["window_launches"])
            live.append(tuple(e.live_status()))
            if b == resume_at:
                X, lp, Z, M = e.get_state()
                e.set_state(np.array(X), np.array(lp), np.array(Z[:M]))
        chain, lobj = e.get_history(1, G) if history else (None, None)
        X, lp, Z, M = e.get_state()
        total, from_ballots = e.changed_total(changed_from, G, with_source=True)
        tail = e.changed_total(tail_from(live[-1][0]), G, with_source=True) if tail_from else (None, None)
        return dict(chain=chain, log_obj=lobj, X=np.array(X), logp=np.array(lp), Z=np.array(Z[:M]), M=M, changed=total,
                    from_ballots=from_ballots, changed_tail=tail[0], tail_from_ballots=tail[1], names=names, launches=launches, live=live,
                    layout=layout)
    finally:
        e.close()


def _same_as_oracle(got, ref, what, keys=("chain", "log_obj", "X", "logp", "Z"), changed_from=1):
    same_bits(got, ref, keys=keys, what=what)
    assert got["M"] == ref["M"], what
    assert got["changed"] == int(ref["changed"][changed_from - 1:].sum()), \
        f"{what}: changed_total {got['changed']} (from the ballots: {got['from_ballots']})"


def _set_env(monkeypatch, case):
    for v in case["env"]:
        monkeypatch.setenv(v, "1")


def _mlb_run(demc, oracle, case, layout, lanes_asked, lanes=None, live=True, **kw):
    """One mlb world on the fused (`layout` "fused") or the split layout, names and LIVE status held to the plan.  live = None: a
    split handle that the device may or may not hold in one LIVE launch -- what its LIVE status says decides the plan: LIVE
    pieces as planned, or every piece the non-LIVE form, one launch per K-window."""
    got = engine_run(demc, case, lanes_asked, **kw)
    what = f"{case['name']}, {layout}"
    if live is None:
        live = got["live"][0][0]
    pieces = case["pieces"] if live else [(a, b, t, f.replace("LIVE", "non-LIVE").replace("non-non-", "non-")) for a, b, t, f in case["pieces"]]
    assert got["layout"] == (SPLIT if layout == "split" else bc.MLB_LANES[case["d"]]), what
    assert len(got["names"]) == len(case["pieces"])
    for (a, b, _, form), name, status in zip(pieces, got["names"], got["live"]):
        inst = bc.instantiation(case, layout, form, lanes=lanes)
        assert name == bc.reported_name(inst), f"{what}, generations {a}..{b}: planned {form} {inst}, ran {name}"
        assert status == ((True, 0) if layout == "split" and live else (False, 0)), \
            f"{what}, generations {a}..{b}: LIVE status {status} (a LIVE launch that timed out and was redone did not produce these numbers)"
    if layout == "split" and live:
        assert got["launches"] == list(range(1, len(pieces) + 1)), f"{what}: a piece is one launch: the name read behind it is that launch's"
    elif layout == "split":
        assert got["launches"] == bc.per_window_launches(pieces), f"{what}: one launch per K-window"
    _same_as_oracle(got, bc.oracle_run(oracle, case), what, keys=("chain", "log_obj", "X", "logp", "Z") if kw.get("history", True) else ("X", "logp", "Z"),
                    changed_from=kw.get("changed_from", 1))
    got["went_live"] = bool(live)
    return got


# ---- window_kernel_mlb: the main worlds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", list(bc.MLB_WORLDS))
def test_fused_block_kernels_every_structure_every_form(demc, oracle, monkeypatch, world):
    case = bc.mlb_case(world)
    _set_env(monkeypatch, case)
    _mlb_run(demc, oracle, case, "fused", bc.MLB_LANES[case["d"]])


@pytest.mark.parametrize("world", list(bc.MLB_WORLDS))
def test_split_block_kernels_every_structure_every_form(demc, oracle, monkeypatch, world):
    case = bc.mlb_case(world)
    _set_env(monkeypatch, case)
    assert {p[3] for p in case["pieces"]} == set(bc.FORMS)
    _mlb_run(demc, oracle, case, "split", SPLIT)


# ---- the 32-lane split form: DEMCZ_MLB_L32 is read once per process ---------------------------------------------------------------------
if os.environ.get(L32):
    @pytest.mark.parametrize("world", bc.L32_WORLDS)
    def test_thirty_two_lanes_every_structure_every_form(demc, oracle, monkeypatch, world):
        """(Collected only in a process that has the switch: the child of the test below.)  lanes_per_chain = 0 takes the split
        layout with 32 lanes per chain for d = 20 in blocks; the four 32-lane forms: LIVE x group-start mask."""
        case = bc.mlb_case(world)
        _set_env(monkeypatch, case)
        got = _mlb_run(demc, oracle, case, "split", 0, lanes=32)
        assert all(n.startswith("demcz::window_kernel_mlb<MVNORMAL, 20, 32, true, ") for n in got["names"]), got["names"]


def test_the_thirty_two_lane_forms_in_a_child_process():
    env = dict(os.environ)
    env[L32] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_block_forms.py",
                        "-k", "test_thirty_two_lanes_every_structure_every_form"], cwd=str(ROOT), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert "%d passed" % len(bc.L32_WORLDS) in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


# ---- four-wave workgroups of the split layout --------------------------------------------------------------------------------------------
_CUS = []


def _device_cus():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once.  In a process where the library has brought up the HIP
    runtime first, torch may find no device: then a child process asks."""
    if not _CUS:
        import torch
        if torch.cuda.is_available():
            _CUS.append(int(torch.cuda.get_device_properties(0).multi_processor_count))
        else:
            r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-1000:]
            _CUS.append(int(r.stdout.split()[-1]))
    return _CUS[0]


@pytest.mark.parametrize("world,sign", bc.FOUR_WAVE_WORLDS, ids=["%s-%s" % (w, "over" if s > 0 else "under") for w, s in bc.FOUR_WAVE_WORLDS])
def test_four_wave_workgroups(demc, oracle, monkeypatch, world, sign):
    """Nothing the library reports exposes the workgroup shape: this asserts the inequality demcz_create decides it by -- chain
    waves >= 4 x the device's CUs -- and relies on it.  The last workgroup is partly filled.  One workgroup more than the device
    has CUs ("over") or one per CU ("under"): LIVE where the device holds them together -- block_cases.FOUR_WAVE_LIVE must, at 8
    and at 16 lanes -- otherwise one launch per K-window, by the handle's own LIVE status."""
    cus = _device_cus()
    case = bc.four_wave_case(world, sign, cus)
    L = bc.MLB_LANES[case["d"]]
    assert bc.chain_waves(case) >= 4 * cus and case["N"] % (4 * (64 // L)) != 0
    _set_env(monkeypatch, case)
    got = _mlb_run(demc, oracle, case, "split", SPLIT, live=True if (world, sign) in bc.FOUR_WAVE_LIVE else None)
    print(case["name"], "N", case["N"], "CUs", cus, "LIVE" if got["went_live"] else "one launch per K-window")


# ---- one lane per chain --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", list(bc.ONE_LANE_WORLDS))
def test_one_lane_block_kernels_every_target(demc, oracle, world):
    case = bc.one_lane_case(world)
    got = engine_run(demc, case, 1)
    assert got["layout"] == 1
    want = bc.one_lane_name(case["kind"], case["d"])
    assert got["names"] == [want] * len(case["pieces"]), (want, got["names"])
    assert set(got["live"]) == {(False, 0)}
    _same_as_oracle(got, bc.oracle_run(oracle, case), world)


def test_more_blocks_than_the_lane_kernels_hold_fall_back_to_one_lane(demc, oracle):
    case = bc.many_blocks_case()
    assert len(case["blocks"]) > bc.MLB_MAX_BLOCKS
    got = engine_run(demc, case, 0)
    assert got["layout"] == 1, "lanes_per_chain = 0 with 65 blocks must take one lane per chain"
    assert set(got["names"]) == {bc.one_lane_name("mvn", 10)}
    _same_as_oracle(got, bc.oracle_run(oracle, case), case["name"])


# ---- named edges ------------------------------------------------------------------------------------------------------------------------------
def _layouts(case):
    return (("fused", bc.MLB_LANES[case["d"]]), ("split", SPLIT))


@pytest.mark.parametrize("layout", ["fused", "split"])
@pytest.mark.parametrize("world,N", bc.TINY)
def test_tiny_populations(demc, oracle, world, N, layout):
    """Idle chain groups in the only wave."""
    case = bc.edge_case(world, N=N)
    _mlb_run(demc, oracle, case, layout, dict(_layouts(case))[layout])


@pytest.mark.parametrize("layout", ["fused", "split"])
@pytest.mark.parametrize("world", bc.NO_HISTORY_WORLDS)
def test_no_history_kept(demc, oracle, world, layout):
    """Gcap = 0: state, archive and the ballots' changed_total."""
    case = bc.edge_case(world)
    got = _mlb_run(demc, oracle, case, layout, dict(_layouts(case))[layout], history=False)
    assert got["from_ballots"]


@pytest.mark.parametrize("layout", ["fused", "split"])
@pytest.mark.parametrize("world", bc.ZERO_TEMPERATURE_WORLDS)
def test_zero_tiny_and_huge_temperatures(demc, oracle, world, layout):
    case = bc.zero_temperature_case(world)
    assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist())
    _mlb_run(demc, oracle, case, layout, dict(_layouts(case))[layout])


@pytest.mark.parametrize("layout", ["one", "fused", "split"])
def test_a_parameter_in_no_block_keeps_its_starting_bits(demc, oracle, layout):
    case = bc.left_out_case()
    if layout == "one":
        got = engine_run(demc, case, 1)
        assert got["layout"] == 1
        _same_as_oracle(got, bc.oracle_run(oracle, case), case["name"])
    else:
        got = _mlb_run(demc, oracle, case, layout, dict(_layouts(case))[layout])
    X0 = case["problem"]["Zinit"][-case["N"]:]
    for p in (2, 4):
        assert (got["chain"][:, p, :].view(np.uint64) == np.ascontiguousarray(X0[:, p]).view(np.uint64)[:, None]).all(), f"parameter {p} moved"
    assert (got["chain"][:, 0, -1] != X0[:, 0]).any()


@pytest.mark.parametrize("layout", ["fused", "split"])
@pytest.mark.parametrize("world", bc.RESUMED_WORLDS)
def test_a_run_carried_on_after_set_state(demc, oracle, world, layout):
    """The incremental form rebuilds its cached partials at every launch's start from the state it is given.  (demcz_set_state
    opens the history window anew: its log-densities become what generation 1 is counted against, so changed_total is asked
    from the generation behind the hand-back.)"""
    case = bc.resumed_case(world)
    _mlb_run(demc, oracle, case, layout, dict(_layouts(case))[layout], resume_at=bc.RESUME_AT, changed_from=bc.RESUME_AT + 1)
