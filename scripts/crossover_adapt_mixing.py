"""What the adaptation of the class weights buys: the experiment of scripts/crossover_mixing.py (correlated MvNormal at d = 30,
N = 1024 chains on the one-lane layout, the same archive start, seed, length and statistics over the second half) with a third
run -- crossover (3, 3) with the weights adapted over the discarded first half (every = 100, until = generations / 2) -- beside
the two rows of that script, re-measured in the same session as its yardsticks.

Reported for the adapted run in addition: the final shares of the classes, the jump distance per step tried by class (what the
weights follow), and the updates made.  No threshold: the numbers go into DESIGN.md section 4.20 as measured.
usage: python scripts/crossover_adapt_mixing.py [generations]      (one JSON object; profiles/crossover_adapt_mixing.txt)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import demc_jl_amd as demc                                  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
N, D, K = 1024, 30, 10
EVERY = 100


def one(w, Z0, crossover, adapt=None):
    e = demc.HipEngine(N=N, d=D, K=K, Mcap=Z0.shape[0] + N * (G // K + 1), Gcap=G, blockindex=[range(D)], eps_scale=w["eps_scale"], seed=7,
                       target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        if crossover:
            e.set_crossover(*crossover)
        if adapt:
            e.set_crossover_adapt(*adapt)
        t0 = time.perf_counter()
        e.run(1, G, w["gamma"])
        e.synchronize()
        wall = time.perf_counter() - t0
        half = G // 2
        ess = e.ess(half + 1, G)
        acc = e.accept_ratio(half + 1, G)
        draws = N * (G - half)
        out = dict(kernel=e.kernel_name(), generations=G, wall_s=round(wall, 3), launches=e.info()["window_launches"],
                   accept_ratio_mean=round(float(acc.mean()), 4),
                   ess_min=round(float(ess.ess.min()), 1), ess_median=round(float(np.median(ess.ess)), 1),
                   ess_min_per_1000_evaluations=round(1000.0 * float(ess.ess.min()) / draws, 3),
                   ess_median_per_1000_evaluations=round(1000.0 * float(np.median(ess.ess)) / draws, 3),
                   ess_converged=int(ess.converged.sum()), draws=draws)
        if crossover:
            c = e.crossover
            out.update(tried=[int(v) for v in c.tried], accepted=[int(v) for v in c.accepted], accept_rate=[round(float(v), 4) for v in c.accept_rate])
        if adapt:
            a = e.crossover_adapt
            out.update(every=a.every, until=a.until, updates=a.updates, weights=[int(v) for v in a.weights],
                       shares=[round(float(v), 4) for v in a.shares], jump_per_try=[round(float(v), 4) for v in a.jump_per_try],
                       rsd_min_max=[round(float(a.rsd.min()), 4), round(float(a.rsd.max()), 4)])
        return out
    finally:
        e.close()


def main():
    w = demc.workloads.mvnormal_problem(D, N)
    r = np.random.default_rng(30)
    Z0 = np.asfortranarray(w["mu"] + 2.0 * r.standard_normal((N + 10 * D, D)) @ np.linalg.cholesky(w["Sigma"]).T)
    until = (G // 2 // EVERY) * EVERY
    print(json.dumps(dict(what="MvNormal d=30 N=1024, one-lane layout, second half of the run", K=K, gamma=w["gamma"],
                          full_block=one(w, Z0, None), crossover_3_3=one(w, Z0, (3, 3)),
                          crossover_3_3_adapted=one(w, Z0, (3, 3), (EVERY, until))), indent=1))


if __name__ == "__main__":
    main()
