"""Crossover generations (demcz_set_crossover): what a K-window of crossover generations costs against the same K-window of the
full-block move on the one-lane kernel (window_kernel<T, D, true>, which this feature leaves as it was, instruction for
instruction).

Every K-window (K = 10 generations, the last one appends) is a demcz_run call of its own, so that demcz_set_kernel_timing brackets
every launch by itself; a fresh handle per column (crossover is set before the first generation) runs WARMUP + LAUNCHES windows,
and the medians (and min..max) of the timed brackets are reported -- clocks as found, nothing pinned.  No history is kept
(Gcap = 0): the kernels would store the same N (d + 1) doubles a generation.

Points: MvNormal N = 1024, d = 5; MvNormal N = 131072, d = 20; a program target (Rosenbrock, d = 7) at N = 1024; each with
crossover (3, 3) and (1, 1).
usage: python scripts/crossover_time.py [launches]      (one JSON object; profiles/crossover_time.txt)"""
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


def column(label, target, Z0, N, d, eps, gamma, crossover):
    """WARMUP + LAUNCHES K-window calls on a fresh handle; the timed brackets' durations in microseconds"""
    total = WARMUP + LAUNCHES
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Z0.shape[0] + N * (total + 1), Gcap=0, blockindex=[range(d)], eps_scale=eps, seed=1,
                       target=target, lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        if crossover:
            e.set_crossover(*crossover)
        for w in range(WARMUP):
            e.run(w * K + 1, (w + 1) * K, gamma)
        e.synchronize()
        e.set_kernel_timing(True)
        for w in range(WARMUP, total):
            e.run(w * K + 1, (w + 1) * K, gamma)
        e.synchronize()
        n, _ = e.get_kernel_time()
        _, dur = e.get_kernel_time_series()
        e.set_kernel_timing(False)
        assert n == LAUNCHES and len(dur) == LAUNCHES
        us = 1e3 * np.asarray(dur)
        out = dict(kernel=e.kernel_name(), median_us=round(float(np.median(us)), 2), min_us=round(float(us.min()), 2), max_us=round(float(us.max()), 2))
        if crossover:
            c = e.crossover
            out["accept_rate"] = [round(float(v), 4) for v in c.accept_rate]
        return out
    finally:
        e.close()


def point(label, target, Z0, N, d, eps, gamma):
    plain = column(label, target, Z0, N, d, eps, gamma, None)
    row = dict(point=label, N=N, d=d, launches=LAUNCHES, generations_per_launch=K, full_block=plain)
    for cr in ((3, 3), (1, 1)):
        col = column(label, target, Z0, N, d, eps, gamma, cr)
        col["ratio_of_medians"] = round(col["median_us"] / plain["median_us"], 3)
        row[f"crossover_{cr[0]}_{cr[1]}"] = col
    return row


def main():
    rows = []
    for N, d in ((1024, 5), (131072, 20)):
        w = demc.workloads.mvnormal_problem(d, N)
        rows.append(point(f"MvNormal N={N} d={d}", w["target"], np.asfortranarray(w["Zinit"]), N, d, w["eps_scale"], w["gamma"]))
    N, d = 1024, 7
    Z0 = np.asfortranarray(0.5 * np.random.default_rng(107).standard_normal((N, d)) + 0.5)
    rows.append(point(f"program (Rosenbrock) N={N} d={d}", demc.ProgramTarget(ROSENBROCK, d), Z0, N, d, 1e-3 * np.ones(d), 0.5))
    print(json.dumps(dict(what="kernel time of K-window launches, demcz_set_kernel_timing", library=str(demc._lib.LIB_PATH.name), K=K,
                          warmup=WARMUP, rows=rows), indent=1))


if __name__ == "__main__":
    main()
