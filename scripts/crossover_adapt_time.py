"""Adaptation of the crossover class weights (demcz_set_crossover_adapt): what the ADAPT instantiation of the crossover kernel costs
against window_kernel_cr<T, D> of the same build (the parent commit's kernel, unchanged instruction for instruction), with the
accumulation on and off, and what one cr_adapt_kernel costs.

As scripts/crossover_time.py: every K-window (K = 10 generations, the last one appends) is a demcz_run call of its own bracketed by
demcz_set_kernel_timing; a fresh handle per column runs WARMUP + LAUNCHES windows; medians and min..max of the timed brackets,
clocks as found, no history kept.  Columns, all with crossover (3, 3):
  plain       no adaptation: window_kernel_cr<T, D>
  accumulate  every = until = 16000: the ADAPT kernel, accumulating in every timed window, no update inside the timing
  frozen      every = until = 10: one update in the first warm-up window, then the ADAPT kernel with accumulate off
  updating    every = 10, until = 16000: accumulating, and one cr_adapt_kernel behind every timed window, inside its bracket
The same three points as scripts/crossover_time.py.
usage: python scripts/crossover_adapt_time.py [launches]      (one JSON object; profiles/crossover_adapt_time.txt)"""
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
COLUMNS = (("plain", None), ("accumulate", (16000, 16000)), ("frozen", (10, 10)), ("updating", (10, 16000)))


def column(target, Z0, N, d, eps, gamma, adapt):
    total = WARMUP + LAUNCHES
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Z0.shape[0] + N * (total + 1), Gcap=0, blockindex=[range(d)], eps_scale=eps, seed=1,
                       target=target, lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        e.set_crossover(3, 3)
        if adapt:
            e.set_crossover_adapt(*adapt)
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
        if adapt:
            a = e.crossover_adapt
            out.update(updates=a.updates, shares=[round(float(v), 4) for v in a.shares])
        return out
    finally:
        e.close()


def point(label, target, Z0, N, d, eps, gamma):
    row = dict(point=label, N=N, d=d, launches=LAUNCHES, generations_per_launch=K)
    for name, adapt in COLUMNS:
        row[name] = column(target, Z0, N, d, eps, gamma, adapt)
        row[name]["ratio_to_plain"] = round(row[name]["median_us"] / row["plain"]["median_us"], 3)
    row["one_update_us"] = round(row["updating"]["median_us"] - row["accumulate"]["median_us"], 2)
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
