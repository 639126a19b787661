"""What quantiles and the best draw cost on C2 (MvNormal d = 5, N = 1024, K = 10) after one 1000-generation slab and after the full
25-slab run, over the same window of the resident history:

  1. demcz_rhat                                  (the yardstick: a read-once reduction of the same bytes)
  2. demcz_quantiles, probs (0.025, 0.5, 0.975)  (eight counting passes, each reading the window once)
  3. demcz_best                                  (one pass over log_obj)
  4. the host route a user has without them: get_history + np.quantile per parameter

Wall clock around each library call (every call ends with the stream synchronised), three warm-up calls, then `reps` timed ones:
median and min .. max.  The host route is timed once per window (its download alone dwarfs the others).  Also printed: one
counting pass per shift (demcz_select_counts with the prefixes the median's walk has at that shift, one per parameter), which
tells a pass that is bound by the loads from one that is bound by its hot bins, and the largest share of a wave's draws in one bin.

    python scripts/quantile_time.py [reps] [slabs]      -> profiles/r09_quantile_time.txt
"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import demc_jl_amd as demc                                           # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
slabs = int(sys.argv[2]) if len(sys.argv) > 2 else 25
d, N, K, every = 5, 1024, 10, 1000
G = slabs * every
PROBS = (0.025, 0.5, 0.975)


def timed(f, n=reps, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def host_route(e, a, b):
    t0 = time.perf_counter()
    chain, _ = e.get_history(a, b)
    t1 = time.perf_counter()
    q = np.stack([np.quantile(chain[:, p, :], PROBS) for p in range(d)])
    t2 = time.perf_counter()
    return q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, chain.nbytes


w = demc.workloads.mvnormal_problem(d, N)
M0 = w["Zinit"].shape[0]
e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=1,
                   target=w["target"])
e.set_state(w["Zinit"][-N:], None, w["Zinit"])
print(f"C2: MvNormal d={d}, N={N}, K={K}; probs {PROBS}; {reps} timed calls after 3 warm-up calls, wall clock in us: median (min .. max)")
done = 0
for upto in sorted({every, G}):
    e.run(done + 1, upto, w["gamma"])
    e.synchronize()
    done = upto
    S = N * upto
    r = e.quantiles(1, upto, PROBS, with_order_stats=True)
    print(f"\nwindow 1..{upto} ({upto // every} slab(s), S = {S} draws per parameter, {S * d * 8 / 1e6:.0f} MB)")
    print(f"  q {np.round(r.q, 4).tolist()}")
    b = e.best(1, upto)
    print(f"  best {b.bestval:.6g} at chain {b.chain}, generation {b.generation}")
    t_rhat = timed(lambda: e.rhat(1, upto))
    t_q = timed(lambda: e.quantiles(1, upto, PROBS))
    t_q1 = timed(lambda: e.quantiles(1, upto, (0.5,)))
    t_q16 = timed(lambda: e.quantiles(1, upto, tuple(np.linspace(0.0, 1.0, 16))))
    t_best = timed(lambda: e.best(1, upto))
    print("  demcz_rhat                       %9.1f (%.1f .. %.1f)" % t_rhat)
    print("  demcz_quantiles, 3 probs         %9.1f (%.1f .. %.1f)   = %.1f x demcz_rhat (eight passes; the yardstick allows 16 x)" % (t_q + (t_q[0] / t_rhat[0],)))
    print("  demcz_quantiles, 1 prob          %9.1f (%.1f .. %.1f)" % t_q1)
    print("  demcz_quantiles, 16 probs        %9.1f (%.1f .. %.1f)" % t_q16)
    print("  demcz_best                       %9.1f (%.1f .. %.1f)" % t_best)
    # one pass per shift along the median's walk
    prefix = np.zeros((d, 1), dtype=np.uint64)
    rank = np.full((d, 1), (S - 1) // 2, dtype=np.int64)
    for shift in range(56, -8, -8):
        counts, _ = e.select_counts(1, upto, shift, prefix)
        t = timed(lambda: e.select_counts(1, upto, shift, prefix), n=max(5, reps // 2))
        share = counts.max(axis=2)[:, 0] / np.maximum(1, counts.sum(axis=2)[:, 0])
        print("  demcz_select_counts, shift %2d    %9.1f (%.1f .. %.1f)   draws under the prefix %s, largest bin's share %s"
              % ((shift,) + t + (counts.sum(axis=2)[:, 0].tolist(), np.round(share, 3).tolist())))
        prefix, rank = demc.select_step(counts, prefix, rank)
    h, t_dl, t_np, nbytes = host_route(e, 1, upto)
    diff = np.max(np.abs(h - r.q) / np.maximum(np.abs(r.lower), np.abs(r.upper)))
    print(f"  host route                       {(t_dl + t_np) * 1e3:9.1f}   = get_history {t_dl:.1f} ms ({nbytes / 1e6:.0f} MB) + np.quantile {t_np:.1f} ms;"
          f" max |q - q_device| = {diff / 2.0 ** -53:.2f} units of 2^-53 max(|a|, |b|)")
e.close()
