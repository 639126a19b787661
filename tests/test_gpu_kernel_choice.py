"""GPU: which window kernel a handle launches, pinned.

A table of handle configurations that between them reach every arm of the library's kernel choice (one lane per chain, the fused
8 / 16-lane layouts, the split layouts with their replicated, cooperating, block-update and wave-per-chain consumers, program
targets on both of their layouts, and what lanes_per_chain = 0 selects at several populations).  Each runs three pieces --
generations 1..4K in one call, three more, then 2K tempered ones -- and after each piece what the handle says about itself is
compared, field for field, with tests/golden/kernel_choice.json: the kernel's name, the launch counters, the LIVE status, the
layout and the number of window launches; at the end a SHA-256 over the bytes of the state (X, logp, M, Z[:M]).  Results are
bit-deterministic, so nothing here has a tolerance.

The fixture records what the library did at the commit BEFORE the kernel choice was gathered into one resolver:
    python tests/test_gpu_kernel_choice.py --record [path]
writes it (default: the fixture's path).  It is recorded once, from that earlier commit with this file dropped in, never from the
code under test.  Cases that need an environment switch (DEMCZ_PS_DUAL, DEMCZ_PW_MFMA, ...) are left to the tests that start a
process for them."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

import demc_jl_amd as demc
from demc_jl_amd import _lib
from program_texts import ROSENBROCK

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "kernel_choice.json"
SPLIT, WAVE, PROGRAM_WAVE = _lib.LAYOUT_SPLIT, _lib.LAYOUT_SPLIT_WAVE, _lib.LAYOUT_PROGRAM_WAVE
ML_COOP_MAX_OBS = 1536          # demcz_kernels_ml.h


def _halves(d, cut):
    return [range(0, cut), range(cut, d)]


# id -> (target kind, d, N, K, lanes_per_chain, blocks (None: one full block), observations of a regression target)
CASES = {
    # one lane per chain
    "lane1_mvn_d5": ("mvn", 5, 64, 5, 1, None, 0),                       # window_kernel<MVNORMAL, 5, true>
    "lane1_mvn_d7": ("mvn", 7, 64, 5, 1, None, 0),                       # window_kernel_generic
    "lane1_mvn_d5_blocks": ("mvn", 5, 64, 5, 1, _halves(5, 2), 0),       # window_kernel<MVNORMAL, 5, false>
    "lane1_iso_d10": ("iso", 10, 64, 5, 1, None, 0),
    "lane1_iso_d7": ("iso", 7, 64, 5, 1, None, 0),
    "lane1_lr_d10": ("lr", 10, 64, 5, 1, None, 90),
    "lane1_lr_d26": ("lr", 26, 64, 5, 1, None, 90),
    "lane1_lr_d7": ("lr", 7, 64, 5, 1, None, 90),
    "lane1_program_d7": ("prog", 7, 64, 5, 1, None, 0),
    # 8 / 16 lanes per chain, fused
    "ml8_mvn_d5": ("mvn", 5, 100, 5, 8, None, 0),
    "ml16_mvn_d20": ("mvn", 20, 100, 5, 16, None, 0),
    "ml8_iso_d10": ("iso", 10, 100, 5, 8, None, 0),
    "ml16_lr_d10": ("lr", 10, 100, 5, 16, None, 90),                     # window_kernel_lr16<10, false, false>
    "ml16_lr_d7_coop": ("lr", 7, 100, 5, 16, None, 90),                  # helper waves
    "ml16_lr_d7_nocoop": ("lr", 7, 100, 5, 16, None, ML_COOP_MAX_OBS + 64),
    "mlb8_mvn_d5": ("mvn", 5, 100, 5, 8, _halves(5, 2), 0),              # sums cut at the block boundaries
    "mlb8_mvn_d6": ("mvn", 6, 100, 5, 8, [[0, 2, 4], [1, 3, 5]], 0),     # interleaved blocks: not grouped
    "mlb8_mvn_d10": ("mvn", 10, 100, 5, 8, _halves(10, 5), 0),
    "mlb16_mvn_d20_4x5": ("mvn", 20, 100, 5, 16, [range(0, 5), range(5, 10), range(10, 15), range(15, 20)], 0),   # incremental form
    "mlb16_mvn_d20_unequal": ("mvn", 20, 100, 5, 16, _halves(20, 8), 0),                                          # group-start mask
    # DEMCZ_LAYOUT_SPLIT
    "split_mvn_d5": ("mvn", 5, 100, 5, SPLIT, None, 0),                  # pc8
    "split_iso_d10": ("iso", 10, 100, 5, SPLIT, None, 0),
    "split_mvn_d20": ("mvn", 20, 100, 5, SPLIT, None, 0),                # ml, REC
    "split_lr_d10_lr8s": ("lr", 10, 256, 5, SPLIT, None, 90),            # at most one workgroup per CU
    "split_lr_d10_lr16": ("lr", 10, 4096, 5, SPLIT, None, 90),
    "split_mvn_d10_blocks": ("mvn", 10, 100, 5, SPLIT, _halves(10, 5), 0),      # mlb, REC
    "split_mvn_d20_4x5": ("mvn", 20, 100, 5, SPLIT, [range(0, 5), range(5, 10), range(10, 15), range(15, 20)], 0),
    # DEMCZ_LAYOUT_SPLIT_WAVE
    "wave_mvn_d2": ("mvn", 2, 100, 5, WAVE, None, 0),                    # ps2
    "wave_mvn_d3": ("mvn", 3, 100, 5, WAVE, None, 0),
    "wave_mvn_d4": ("mvn", 4, 100, 5, WAVE, None, 0),
    "wave_mvn_d5": ("mvn", 5, 100, 5, WAVE, None, 0),
    "wave_mvn_d5_K7": ("mvn", 5, 100, 7, WAVE, None, 0),                 # ps
    "wave_mvn_d6": ("mvn", 6, 100, 5, WAVE, None, 0),                    # pw: regular, then general
    "wave_mvn_d20": ("mvn", 20, 100, 5, WAVE, None, 0),
    "wave_mvn_d32": ("mvn", 32, 100, 5, WAVE, None, 0),
    "wave_iso_d6": ("iso", 6, 100, 5, WAVE, None, 0),
    "wave_mvn_d6_K7": ("mvn", 6, 100, 7, WAVE, None, 0),                 # pw: general only
    # DEMCZ_LAYOUT_PROGRAM_WAVE
    "program_wave_d7": ("prog", 7, 100, 5, PROGRAM_WAVE, None, 0),
    # lanes_per_chain = 0
    "auto_mvn_d5_N128": ("mvn", 5, 128, 5, 0, None, 0),
    "auto_mvn_d5_N2048": ("mvn", 5, 2048, 5, 0, None, 0),
    "auto_mvn_d5_N4096": ("mvn", 5, 4096, 5, 0, None, 0),
    "auto_mvn_d20_N1024": ("mvn", 20, 1024, 5, 0, None, 0),
}


def _problem(kind, d, N, nobs):
    if kind == "mvn":
        return demc.workloads.mvnormal_problem(d, N)
    if kind == "iso":
        return demc.workloads.iso_quad_problem(d, N)
    if kind == "lr":
        return demc.workloads.linreg_problem(d, N, nobs=nobs)
    r = np.random.default_rng(100 + d)
    return dict(target=demc.ProgramTarget(ROSENBROCK, d), Zinit=np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5),
                eps_scale=1e-3 * np.ones(d), gamma=0.8)


def _observe(e):
    e.synchronize()
    info = e.info()
    return dict(kernel_name=e.kernel_name(), kernel_counts=e.kernel_counts(), live_status=list(e.live_status()),
                lanes_per_chain=info["lanes_per_chain"], window_launches=info["window_launches"])


def observe_case(case):
    kind, d, N, K, lanes, blocks, nobs = CASES[case]
    w = _problem(kind, d, N, nobs)
    G = 6 * K + 3
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=blocks or [range(d)],
                       eps_scale=w["eps_scale"], seed=20261018, target=w["target"], lanes_per_chain=lanes)
    try:
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        pieces = []
        e.run(1, 4 * K, w["gamma"])
        pieces.append(_observe(e))
        e.run(4 * K + 1, 4 * K + 3, w["gamma"])
        pieces.append(_observe(e))
        T = np.array([demc.tempbaseline(g, 2 * K, 3, 1e-3) for g in range(1, 2 * K + 1)])
        e.run(4 * K + 4, G, w["gamma"], temperature=T)
        pieces.append(_observe(e))
        X, lp, Z, M = e.get_state()
        digest = hashlib.sha256()
        for a in (np.array(X), np.array(lp), np.array([M], dtype=np.int64), np.array(Z[:M])):
            digest.update(a.tobytes())
    finally:
        e.close()
    return dict(pieces=pieces, sha256=digest.hexdigest())


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def test_the_fixture_covers_the_table(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_choice_is_the_recorded_one(recorded, case):
    got, want = observe_case(case), recorded[case]
    for i, (g, r) in enumerate(zip(got["pieces"], want["pieces"])):
        for field in r:
            assert g[field] == r[field], f"{case}, piece {i}: {field}: {g[field]!r}, recorded {r[field]!r}"
    assert len(got["pieces"]) == len(want["pieces"])
    assert got["sha256"] == want["sha256"], f"{case}: the state after the run differs from the recorded one"


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_kernel_choice.py --record [path]")
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else FIXTURE
    table = {}
    for name in CASES:
        table[name] = observe_case(name)
        print(name, table[name]["pieces"][0]["kernel_name"], "|", table[name]["pieces"][1]["kernel_name"], "|",
              table[name]["pieces"][2]["kernel_name"], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out}")
