"""GPU: the window launches a sequence of demcz_run calls is cut into, pinned.

tests/test_gpu_kernel_choice.py pins which kernel a handle launches; this table pins the launch SCHEDULE on the paths that table does
not reach: calls that start mid-window, a call longer than the one before it (the prepared draws are shorter than the span), a
one-window call, the two-chain handle going from regular launches to irregular ones and back, an append lag with a call that ends
mid-batch, caller-owned appends, an offset of the random streams, and demcz_run_checked's grouped calls with their next-launch
hint.  After every call what the handle says about itself is compared, field for field, with tests/golden/run_schedule.json: the
number of window launches, the kernel's name, the launch counters and the LIVE status; at the end a SHA-256 over the bytes of
X, logp, M, Z[:M] and the chain and log_obj history.  Results are bit-deterministic, so nothing here has a tolerance.

The fixture records what the library did at the commit BEFORE the schedule of demcz_run moved into demcz_run_plan.h:
    python tests/test_gpu_run_schedule.py --record [path]
writes it (default: the fixture's path).  It is recorded once, from that earlier commit with this file dropped in, never from the
code under test."""
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

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "run_schedule.json"
SPLIT, WAVE = _lib.LAYOUT_SPLIT, _lib.LAYOUT_SPLIT_WAVE
SEED = 20261019

# id -> dict(d, N, K, lanes, blocks (None: one full block), calls [(g_from, g_to)], and what sets the case apart:
#            lag, external, rng_offset, tempered (index of the call that is given temperatures), checked (every))
CASES = {
    # a mid-window start, a call longer than the one before, a one-window call
    "wave_d5_K5": dict(d=5, N=100, K=5, lanes=WAVE, calls=[(1, 20), (21, 23), (24, 120), (121, 125)]),
    # the two-chain handle lanes_per_chain = 0 picks: regular launches, irregular ones, regular ones again (tempered)
    "dual_d5_K10_N2048": dict(d=5, N=2048, K=10, lanes=0, calls=[(1, 40), (41, 43), (44, 50), (51, 90)], tempered=3),
    "wave_d6_K5": dict(d=6, N=100, K=5, lanes=WAVE, calls=[(1, 20), (21, 22), (23, 60)]),
    "split_d20_4x5": dict(d=20, N=100, K=5, lanes=SPLIT, blocks=[range(0, 5), range(5, 10), range(10, 15), range(15, 20)],
                          calls=[(1, 30), (31, 33)]),
    # an append lag of two batches; 21..27 ends mid-batch
    "lane1_lag2": dict(d=5, N=100, K=5, lanes=1, lag=2, calls=[(1, 20), (21, 27), (28, 60)]),
    "wave_lag2": dict(d=5, N=100, K=5, lanes=WAVE, lag=2, calls=[(1, 20), (21, 27), (28, 60)]),      # no LIVE launches: one per batch
    # caller-owned appends: one K-window per call, the caller appends the current state after each
    "lane1_external": dict(d=5, N=100, K=5, lanes=1, external=True, calls=[(5 * i + 1, 5 * i + 5) for i in range(6)]),
    "wave_rng_offset": dict(d=5, N=100, K=5, lanes=WAVE, rng_offset=37, calls=[(1, 20), (21, 40)]),
    # demcz_run_checked in monitoring mode: grouped slabs, the next-launch hint
    "wave_checked": dict(d=5, N=100, K=5, lanes=WAVE, checked=20, calls=[(1, 200)]),
}


def _observe(e):
    e.synchronize()
    return dict(kernel_name=e.kernel_name(), kernel_counts=e.kernel_counts(), live_status=list(e.live_status()),
                window_launches=e.info()["window_launches"])


def observe_case(case):
    c = CASES[case]
    d, N, K, calls = c["d"], c["N"], c["K"], c["calls"]
    w = demc.workloads.mvnormal_problem(d, N)
    G = calls[-1][1]
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=c.get("blocks") or [range(d)],
                       eps_scale=w["eps_scale"], seed=SEED, target=w["target"], lanes_per_chain=c["lanes"])
    try:
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        if c.get("lag"):
            e.set_append_lag(c["lag"])
        if c.get("external"):
            e.set_external_append(True)
        if c.get("rng_offset"):
            e.set_rng_offset(c["rng_offset"])
        pieces = []
        for i, (g_from, g_to) in enumerate(calls):
            n = g_to - g_from + 1
            if c.get("checked"):
                g_stop, rhat_max, rhat_last = e.run_checked(g_from, g_to, w["gamma"], c["checked"])
                pieces.append(dict(_observe(e), g_stop=g_stop, n_checks=len(rhat_max),
                                   rhat_max=[float(v).hex() for v in rhat_max], rhat_last=[float(v).hex() for v in rhat_last]))
                continue
            T = np.array([demc.tempbaseline(g, n, 3, 1e-3) for g in range(1, n + 1)]) if c.get("tempered") == i else None
            e.run(g_from, g_to, w["gamma"], temperature=T)
            pieces.append(_observe(e))
            if c.get("external"):
                e.append_rows(e.get_state(with_Z=False)[0])
        X, lp, Z, M = e.get_state()
        chain, log_obj = e.get_history(1, G)
        digest = hashlib.sha256()
        for a in (np.array(X), np.array(lp), np.array([M], dtype=np.int64), np.array(Z[:M]), np.array(chain), np.array(log_obj)):
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
def test_run_schedule_is_the_recorded_one(recorded, case):
    got, want = observe_case(case), recorded[case]
    for i, (g, r) in enumerate(zip(got["pieces"], want["pieces"])):
        for field in r:
            assert g[field] == r[field], f"{case}, call {i}: {field}: {g[field]!r}, recorded {r[field]!r}"
    assert len(got["pieces"]) == len(want["pieces"])
    assert got["sha256"] == want["sha256"], f"{case}: state or history after the run differ from the recorded ones"


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_run_schedule.py --record [path]")
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else FIXTURE
    table = {}
    for name in CASES:
        table[name] = observe_case(name)
        print(name, [p["window_launches"] for p in table[name]["pieces"]], table[name]["pieces"][-1]["kernel_name"], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out}")
