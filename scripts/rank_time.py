"""What the rank-normalised diagnostics cost on C2 (MvNormal d = 5, N = 1024, K = 10) over one 1000-generation slab of the resident
history (S = 1 024 000 draws per parameter), against the route a user has without them:

  1. demcz_rank_diagnostics                         (the whole statistic: rhat_rank, ess_bulk, ess_tail)
  2. its parts, each as its own call:
       demcz_quantiles at (0.05, 0.5, 0.95)          (the median to fold at, the two tail thresholds)
       demcz_rank_normalize, bulk and folded         (each: keys + histograms, the radix sort, rank and score -- the split of one
                                                      call into its kernels is a kernel trace's to give, see below)
       demcz_rank_normalize, raw ranks               (the same sort, no normal score)
       demcz_rhat of the bulk and of the folded scores
       demcz_indicator_le at the two thresholds
       demcz_ess of the bulk scores, and of the 2 d indicator columns (the two tail ESS in one call)
  3. the host route: get_history of the window + average ranks from np.argsort (stable) for the d parameters -- the ranking alone,
     before any score, R-hat or ESS is formed from it

Wall clock around each library call (every call ends with the stream synchronised), three warm-up calls, then `reps` timed ones:
median and min .. max.  The host route is timed once.  The device's ranks are checked against the host's.

    python scripts/rank_time.py [reps]      -> profiles/rank_time.txt
    rocprofv3 --kernel-trace --stats -- python scripts/rank_time.py 3      (per-kernel times: sort passes against rank_score_kernel)
"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import demc_jl_amd as demc                                           # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
d, N, K, G = 5, 1024, 10, 1000


def timed(f, n=reps, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def closing(make):
    def f():
        make().close()
    return f


def host_ranks(x):
    """Average ranks of a 1-d array from one stable argsort."""
    order = np.argsort(x, kind="stable")
    s = x[order]
    first = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    cnt = np.diff(np.append(first, s.size))
    r = np.empty(s.size)
    r[order] = np.repeat(first + (cnt + 1) / 2.0, cnt)
    return r


w = demc.workloads.mvnormal_problem(d, N)
M0 = w["Zinit"].shape[0]
e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=1,
                   target=w["target"])
e.set_state(w["Zinit"][-N:], None, w["Zinit"])
e.run(1, G, w["gamma"])
e.synchronize()
S = N * G
print(f"C2: MvNormal d={d}, N={N}, K={K}; window 1..{G}, S = {S} draws per parameter ({S * d * 8 / 1e6:.0f} MB); {reps} timed calls after 3 "
      f"warm-up calls, wall clock in ms: median (min .. max)")
diag = e.rank_diagnostics(1, G)
print(f"  rhat_rank {np.round(diag.rhat_rank, 5).tolist()}\n  ess_bulk  {np.round(diag.ess_bulk, 1).tolist()}\n  ess_tail  {np.round(diag.ess_tail, 1).tolist()}")
q = e.quantiles(1, G, (0.05, 0.5, 0.95))
rows = [
    ("demcz_rank_diagnostics", lambda: e.rank_diagnostics(1, G)),
    ("demcz_quantiles, 3 probs", lambda: e.quantiles(1, G, (0.05, 0.5, 0.95))),
    ("demcz_rank_normalize, bulk", closing(lambda: e.rank_normalize(1, G))),
    ("demcz_rank_normalize, folded", closing(lambda: e.rank_normalize(1, G, center=q[:, 1]))),
    ("demcz_rank_normalize, raw ranks", closing(lambda: e.rank_normalize(1, G, ranks=True))),
    ("demcz_indicator_le, 2 thresholds", closing(lambda: e.indicator_le(1, G, q[:, [0, 2]]))),
]
times = {}
for name, f in rows:
    times[name] = timed(f)
with e.rank_normalize(1, G) as zb, e.rank_normalize(1, G, center=q[:, 1]) as zf, e.indicator_le(1, G, q[:, [0, 2]]) as ind:
    for name, f in [("demcz_rhat, bulk scores", lambda: zb.rhat(1, G)), ("demcz_rhat, folded scores", lambda: zf.rhat(1, G)),
                    ("demcz_ess, bulk scores", lambda: zb.ess(1, G)), ("demcz_ess, 2 d indicator columns", lambda: ind.ess(1, G)),
                    ("demcz_rhat, the history itself", lambda: e.rhat(1, G))]:
        times[name] = timed(f)
for name, t in times.items():
    print("  %-36s %9.2f (%.2f .. %.2f)" % ((name,) + t))
parts = sum(times[k][0] for k in times if k not in ("demcz_rank_diagnostics", "demcz_rank_normalize, raw ranks", "demcz_rhat, the history itself"))
print(f"  sum of the parts' medians            {parts:9.2f}")

t0 = time.perf_counter()
chain, _ = e.get_history(1, G)
t1 = time.perf_counter()
host = np.empty(chain.shape, order="F")
for p in range(d):
    host[:, p, :] = host_ranks(np.ascontiguousarray(chain[:, p, :]).ravel()).reshape(N, G)
t2 = time.perf_counter()
with e.rank_normalize(1, G, ranks=True) as h:
    same = np.array_equal(h.get(), host)
t_dev = times["demcz_rank_diagnostics"][0]
t_host = (t2 - t0) * 1e3
print(f"  host route                           {t_host:9.2f}   = get_history {(t1 - t0) * 1e3:.1f} ms ({chain.nbytes / 1e6:.0f} MB) + np.argsort "
      f"average ranks {(t2 - t1) * 1e3:.1f} ms; the ranks alone: no score, R-hat or ESS yet")
print(f"  device ranks equal the host's: {same}")
print(f"  demcz_rank_diagnostics / host route = {t_dev / t_host:.3f}   (demcz_rank_normalize, raw ranks / host route = "
      f"{times['demcz_rank_normalize, raw ranks'][0] / t_host:.3f})")
e.close()
