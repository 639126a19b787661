"""What crossover generations buy at a dimension where the full-block step's acceptance is low: a correlated MvNormal at d = 30,
N = 1024 chains on the one-lane layout, run once with the full-block move and once with crossover (3, 3) -- same generations,
same archive start (the target's neighbourhood, overdispersed twofold), same seed.

Reported for both: the mean accept ratio over the second half (HipEngine.accept_ratio), the per-class acceptance of the crossover
run (HipEngine.crossover) and the library's own effective sample size per parameter over the second half (HipEngine.ess), as
minimum and median over the parameters, and per thousand log-density evaluations (both moves evaluate once a generation).
No threshold: the numbers go into DESIGN.md section 4.20 as measured.
usage: python scripts/crossover_mixing.py [generations]      (one JSON object; profiles/crossover_mixing.txt)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import demc_jl_amd as demc                                  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
N, D, K = 1024, 30, 10


def one(w, Z0, crossover):
    e = demc.HipEngine(N=N, d=D, K=K, Mcap=Z0.shape[0] + N * (G // K + 1), Gcap=G, blockindex=[range(D)], eps_scale=w["eps_scale"], seed=7,
                       target=w["target"], lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        if crossover:
            e.set_crossover(*crossover)
        t0 = time.perf_counter()
        e.run(1, G, w["gamma"])
        e.synchronize()
        wall = time.perf_counter() - t0
        half = G // 2
        ess = e.ess(half + 1, G)
        acc = e.accept_ratio(half + 1, G)
        draws = N * (G - half)
        out = dict(kernel=e.kernel_name(), generations=G, wall_s=round(wall, 3), accept_ratio_mean=round(float(acc.mean()), 4),
                   ess_min=round(float(ess.ess.min()), 1), ess_median=round(float(np.median(ess.ess)), 1),
                   ess_min_per_1000_evaluations=round(1000.0 * float(ess.ess.min()) / draws, 3),
                   ess_median_per_1000_evaluations=round(1000.0 * float(np.median(ess.ess)) / draws, 3),
                   ess_converged=int(ess.converged.sum()), draws=draws)
        if crossover:
            c = e.crossover
            out.update(tried=[int(v) for v in c.tried], accepted=[int(v) for v in c.accepted], accept_rate=[round(float(v), 4) for v in c.accept_rate])
        return out
    finally:
        e.close()


def main():
    w = demc.workloads.mvnormal_problem(D, N)
    r = np.random.default_rng(30)
    Z0 = np.asfortranarray(w["mu"] + 2.0 * r.standard_normal((N + 10 * D, D)) @ np.linalg.cholesky(w["Sigma"]).T)
    print(json.dumps(dict(what="MvNormal d=30 N=1024, one-lane layout, second half of the run", K=K, gamma=w["gamma"],
                          full_block=one(w, Z0, None), crossover_3_3=one(w, Z0, (3, 3))), indent=1))


if __name__ == "__main__":
    main()
