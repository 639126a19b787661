"""GPU: the wave-per-chain kernels of d = 2..5 and the replicated consumer, every instantiation, bit for bit against the oracle.

window_kernel_ps2 (regular launches, one chain to a wave), window_kernel_ps2d (two chains to a wave) and the general
window_kernel_ps exist for d = 2..5 x LIVE x TEMPER, each dimension with constants of its own (demcz_kernels_ps2.h: the row
strides of 2 / 4 / 8 doubles, the fields of a pass's DMA, the temperature field); window_kernel_pc8 for MvNormal d = 2..10 and the
isotropic quadratic d = 10.  tests/small_wave_cases.py holds the worlds: per d one handle of each kind whose schedule reaches
every form, in which -- by the oracle alone, tests/test_small_wave_cases.py -- every accept / reject outcome of a pass occurs in
every form and, with two chains to a wave, in either half of the wave.  The kernel names asserted here are all 16 + 16 + 16
instantiations of the three wave kernels at d = 2..5 and all 40 of window_kernel_pc8
(test_small_wave_cases.test_every_instantiation_appears_in_a_planned_kernel_name).  No tolerance anywhere."""
import pytest

import dimension_cases as dc
import small_wave_cases as sw
from helpers import SPLIT, SPLIT_WAVE
from test_gpu_every_dimension import _same_as_oracle, engine_run

pytestmark = pytest.mark.gpu


def _run(demc, case, what, history=True):
    got = engine_run(demc, case, SPLIT_WAVE, history=history)
    assert got["layout"] == SPLIT_WAVE
    assert len(got["names"]) == len(case["pieces"])
    for (a, b, _, form), name in zip(case["pieces"], got["names"]):
        want = sw.kernel_name(case["d"], form, case["dual"])
        assert name == want, f"{what}, generations {a}..{b}: planned {form} ({want}), ran {name}"
    return got


@pytest.mark.parametrize("d", sw.DIMS)
def test_one_chain_per_wave_every_dimension_every_form(demc, oracle, d):
    case = sw.small_case(d, False)
    got = _run(demc, case, f"d = {d}")
    assert {p[3] for p in case["pieces"]} == set(sw.ONE_FORMS)
    assert got["launches"] == sw.launches_after(case) == list(range(1, len(case["pieces"]) + 1)), "a piece is one launch"
    assert got["live_status"] == (True, 0), "a LIVE launch timed out and was redone: the LIVE kernels did not produce these numbers"
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"d = {d}")


@pytest.mark.parametrize("d", sw.DIMS)
def test_two_chains_per_wave_every_dimension_every_form(demc, oracle, monkeypatch, d):
    monkeypatch.setenv("DEMCZ_PS_DUAL", "1")
    case = sw.small_case(d, True)
    assert case["N"] % 2 == 1
    got = _run(demc, case, f"two chains to a wave, d = {d}")
    assert {p[3] for p in case["pieces"]} == set(sw.DUAL_FORMS)
    assert got["launches"] == sw.launches_after(case), "a steady piece is one launch, a general one a launch per K-window"
    assert got["live_status"] == (True, 0), "a LIVE launch timed out and was redone: the LIVE kernels did not produce these numbers"
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"two chains to a wave, d = {d}")


@pytest.mark.parametrize("dual", [False, True], ids=["ps2", "ps2d"])
@pytest.mark.parametrize("d", [3, 5])
def test_a_cut_tempered_call_starts_a_launch_at_an_odd_temperature(demc, oracle, monkeypatch, d, dual):
    """The second launch of the tempered call reads its temperatures from arena_temp + 15: the 16-byte pieces of the pass's
    temperature field start 8 bytes off."""
    if dual:
        monkeypatch.setenv("DEMCZ_PS_DUAL", "1")
    case = sw.edge_case(d, 37, dual, sw.CUT_LENGTHS, k=sw.CUT_K)
    got = _run(demc, case, f"d = {d}")
    assert got["launches"] == sw.CUT_LAUNCHES, "the tempered call was not cut behind its fifteenth generation"
    assert got["live_status"] == (True, 0)
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"d = {d}")


@pytest.mark.parametrize("dual", [False, True], ids=["ps2", "ps2d"])
def test_zero_tiny_and_huge_temperatures(demc, oracle, monkeypatch, dual):
    if dual:
        monkeypatch.setenv("DEMCZ_PS_DUAL", "1")
    case = sw.edge_case(3, 37, dual, [(60, True)], temperature=sw.temps_with_zeros(60))
    assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist())
    got = _run(demc, case, "T with zeros")
    assert got["launches"] == [1] and got["live_status"] == (True, 0)
    _same_as_oracle(got, dc.oracle_run(oracle, case), "T with zeros")


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("dual,N", [(dual, N) for dual in (False, True) for N in sw.TINY_POPULATIONS[dual]])
def test_tiny_populations(demc, oracle, monkeypatch, dual, N, d):
    """A workgroup with idle chain waves; with two chains to a wave a wave whose second half shadows.  Row strides 2 and 4."""
    if dual:
        monkeypatch.setenv("DEMCZ_PS_DUAL", "1")
    case = sw.edge_case(d, N, dual, sw.TINY_LENGTHS)
    got = _run(demc, case, f"N = {N}, d = {d}")
    assert got["launches"] == [1, 2, 3, 4] and got["live_status"] == (True, 0)
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"N = {N}, d = {d}")


def test_no_history_kept(demc, oracle):
    """Gcap = 0: every history store of the pass is out of the (empty) buffer's range by design.  State, archive and the ballots'
    changed_total."""
    case = sw.edge_case(4, 37, False, [(40, True)])
    got = _run(demc, case, "Gcap = 0", history=False)
    assert got["launches"] == [1] and got["live_status"] == (True, 0)
    _same_as_oracle(got, dc.oracle_run(oracle, case), "Gcap = 0", keys=("X", "logp", "Z"))


@pytest.mark.parametrize("kind,d", sw.PC8_TARGETS)
def test_replicated_consumer_every_dimension_every_form(demc, oracle, kind, d):
    case = sw.pc8_case(kind, d)
    got = engine_run(demc, case, SPLIT)
    assert got["layout"] == SPLIT
    for (a, b, _, form), name in zip(case["pieces"], got["names"]):
        assert name == sw.pc8_kernel_name(kind, d, form), f"{kind} d = {d}, generations {a}..{b}: planned {form}, ran {name}"
    assert {p[3] for p in case["pieces"]} == set(sw.PC8_FORMS) and len(got["names"]) == len(case["pieces"])
    assert got["launches"] == list(range(1, len(case["pieces"]) + 1)), "a piece is one launch: the name read behind it is that launch's"
    assert got["live_status"] == (True, 0)
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"{kind} d = {d}")
