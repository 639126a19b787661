"""Snooker generations (demcz_set_snooker): what a snooker launch costs against an ordinary one-generation launch of the one-lane
kernel on the same handle shape (window_kernel<T, D, true>, which this feature leaves as it was, instruction for instruction).

Every generation is a demcz_run call of its own, so that demcz_set_kernel_timing brackets every launch by itself; the handle runs
WARMUP + LAUNCHES generations with snooker_every = 0 and then as many with snooker_every = 1, and the medians (and min..max) of
the timed brackets are reported -- clocks as found, nothing pinned.  One generation in K = 10 appends its rows, in both columns.
No history is kept (Gcap = 0): both kernels would store the same N (d + 1) doubles.

Points: MvNormal N = 1024, d = 5; MvNormal N = 131072, d = 20; a program target (Rosenbrock, d = 7) at N = 1024.
usage: python scripts/snooker_time.py [launches]      (one JSON object; profiles/snooker_time.txt)"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import demc_jl_amd as demc                                  # noqa: E402
from program_texts import ROSENBROCK                        # noqa: E402

LAUNCHES = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 40
WARMUP = 10
K = 10


def column(e, g0, gamma):
    """WARMUP + LAUNCHES one-generation calls from generation g0 + 1; the timed brackets' durations in microseconds"""
    for g in range(g0 + 1, g0 + WARMUP + 1):
        e.run(g, g, gamma)
    e.synchronize()
    e.set_kernel_timing(True)
    for g in range(g0 + WARMUP + 1, g0 + WARMUP + LAUNCHES + 1):
        e.run(g, g, gamma)
    e.synchronize()
    n, _ = e.get_kernel_time()
    _, dur = e.get_kernel_time_series()
    e.set_kernel_timing(False)
    assert n == LAUNCHES and len(dur) == LAUNCHES
    return 1e3 * np.asarray(dur), e.kernel_name()


def stats(us):
    return dict(median_us=round(float(np.median(us)), 2), min_us=round(float(us.min()), 2), max_us=round(float(us.max()), 2))


def point(label, target, Z0, N, d, eps, gamma):
    total = 2 * (WARMUP + LAUNCHES)
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Z0.shape[0] + N * (total // K + 2), Gcap=0, blockindex=[range(d)], eps_scale=eps, seed=1,
                       target=target, lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        plain, plain_name = column(e, 0, gamma)
        e.set_snooker(1)
        snk, snk_name = column(e, WARMUP + LAUNCHES, gamma)
        assert e.snooker[3] == WARMUP + LAUNCHES
    finally:
        e.close()
    return dict(point=label, N=N, d=d, launches=LAUNCHES, ordinary=dict(kernel=plain_name, **stats(plain)),
                snooker=dict(kernel=snk_name, **stats(snk)), ratio_of_medians=round(float(np.median(snk) / np.median(plain)), 3))


def main():
    rows = []
    for N, d in ((1024, 5), (131072, 20)):
        w = demc.workloads.mvnormal_problem(d, N)
        rows.append(point(f"MvNormal N={N} d={d}", w["target"], np.asfortranarray(w["Zinit"]), N, d, w["eps_scale"], w["gamma"]))
    N, d = 1024, 7
    Z0 = np.asfortranarray(0.5 * np.random.default_rng(107).standard_normal((N, d)) + 0.5)
    rows.append(point(f"program (Rosenbrock) N={N} d={d}", demc.ProgramTarget(ROSENBROCK, d), Z0, N, d, 1e-3 * np.ones(d), 0.5))
    print(json.dumps(dict(what="kernel time of one-generation launches, demcz_set_kernel_timing", K=K, warmup=WARMUP, rows=rows), indent=1))


if __name__ == "__main__":
    main()
