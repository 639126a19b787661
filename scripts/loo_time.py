"""What PSIS-LOO and WAIC cost on the device: the regression workload's likelihood as a pointwise program, nobs = 1000, d = 10,
N = 1024, one 1000-generation slab resident after `burn` slabs of burn-in (S = 1 024 000 draws; 32 observations a chunk, 32 chunks).

  1. HipEngine.loo end to end (demcz_loo: per chunk demcz_pointwise, demcz_loo_columns, the chunk dropped), wall clock
  2. its stages on one chunk of 32 observations, wall clock: HipEngine.pointwise, then DerivedHistory.loo_columns
     (the kernels themselves: a run of this script under `rocprofv3 --kernel-trace --stats`, summarised by `--trace-summary`)
  3. the host route the library offered before: get_history, then per observation the float64 NumPy restatement of
     tests/loo_reference.py (sort included) -- timed on `host_obs` observations and scaled to nobs, because the whole
     nobs x S matrix is 8 GB

Three warm-up calls (the first compiles the program), then `reps` timed ones: median and min .. max, clocks as found.

    python scripts/loo_time.py [reps] [host_obs] [burn]                 -> profiles/loo_time.txt
    python scripts/loo_time.py --trace-summary KERNEL_STATS.csv         kernel totals of a profiled run, by stage
"""
import csv
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STAGES = (("pointwise", ("pointwise_kernel",)),
          ("sort", ("rank_keys_kernel", "rank_tile_count_kernel", "rank_tile_scan_kernel", "rank_scatter_kernel")),
          ("fit and sums", ("psis_fit_kernel", "loo_sum_kernel", "loo_finish_kernel")))


def trace_summary(path):
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    total_key = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls_key = next(k for k in rows[0] if k.lower() == "calls")
    grand = 0.0
    for stage, kernels in STAGES:
        sub = 0.0
        for kn in kernels:
            hit = [r for r in rows if kn in r[name_key]]
            ns = sum(float(r[total_key]) for r in hit)
            calls = sum(int(r[calls_key]) for r in hit)
            sub += ns
            print(f"    {kn:26s} n={calls:6d}  total {ns / 1e6:10.2f} ms")
        grand += sub
        print(f"  stage {stage:14s} {sub / 1e6:10.2f} ms")
    print(f"  all three stages      {grand / 1e6:10.2f} ms")


if len(sys.argv) > 2 and sys.argv[1] == "--trace-summary":
    trace_summary(sys.argv[2])
    sys.exit(0)

import demc_jl_amd as demc                                           # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_obs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
burn = int(sys.argv[3]) if len(sys.argv) > 3 else 10
d, N, K, G, nobs = 10, 1024, 10, 1000, 1000

SOURCE = f"""
#define NOBS {nobs}
__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)
{{
    const double* row = data + i * DEMCZ_D;
    double mu = 0.0;
#pragma unroll
    for (int p = 0; p < DEMCZ_D; ++p) mu = fma(row[p], x[p], mu);
    const double r = data[(int64_t)NOBS * DEMCZ_D + i] - mu;
    return fma(-0.5 * r, r, -0.9189385332046727);
}}
"""


def fmt(ts, unit="ms"):
    return f"{statistics.median(ts):10.2f} ({min(ts):.2f} .. {max(ts):.2f}) {unit}"


w = demc.workloads.linreg_problem(d, N, nobs=nobs)
M0 = w["Zinit"].shape[0]
e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * ((burn + 1) * G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=1,
                   target=w["target"])
e.set_state(w["Zinit"][-N:], None, w["Zinit"])
for slab in range(burn + 1):                                          # the window slides: the last slab stays resident
    e.set_history_origin(slab * G)
    e.run(slab * G + 1, (slab + 1) * G, w["gamma"])
e.synchronize()
g1, g2 = burn * G + 1, (burn + 1) * G
prog = demc.PointwiseProgram(SOURCE, d, nobs, data=np.concatenate([w["design"].ravel(), w["y"]]))
S = N * G
print(f"regression workload d={d}, N={N}, K={K}, generations {g1}..{g2} on the device; nobs={nobs}; S={S} draws; {reps} timed calls after "
      f"three calls; median (min .. max)")
t0 = time.perf_counter()
rec = e.loo(prog, g1, g2)
print(f"first call (compiles the program)                  {(time.perf_counter() - t0) * 1e3:10.2f} ms")
for _ in range(2):
    e.loo(prog, g1, g2)
whole = []
for _ in range(reps):
    t0 = time.perf_counter()
    rec = e.loo(prog, g1, g2)
    whole.append((time.perf_counter() - t0) * 1e3)
print(f"HipEngine.loo end to end, {nobs} observations        {fmt(whole)}")
print(f"  elpd_loo {rec.elpd_loo:.3f} (se {rec.se_elpd_loo:.3f}), p_loo {rec.p_loo:.3f}, elpd_waic {rec.elpd_waic:.3f}, p_waic {rec.p_waic:.3f}, "
      f"largest khat {np.max(rec.pareto_k):.3f}, threshold {rec.k_threshold:.2f}, {rec.bad_k.size} above it, n_tail {rec.n_tail.min()} .. {rec.n_tail.max()}")
pw, lc_ = [], []
for i in range(3 + reps):
    t0 = time.perf_counter()
    h = e.pointwise(prog, g1, g2, 0, 32)
    t1 = time.perf_counter()
    part = h.loo_columns(g1, g2)
    t2 = time.perf_counter()
    h.close()
    if i >= 3:
        pw.append((t1 - t0) * 1e3)
        lc_.append((t2 - t1) * 1e3)
print(f"one chunk of 32 observations: HipEngine.pointwise    {fmt(pw)}")
print(f"                              loo_columns (sort, fit, sums) {fmt(lc_)}")
print(f"  x {-(-nobs // 32)} chunks: pointwise {statistics.median(pw) * -(-nobs // 32):.1f} ms, loo_columns {statistics.median(lc_) * -(-nobs // 32):.1f} ms")
assert np.array_equal(part.elpd_loo_i, rec.elpd_loo_i[:32])

if host_obs > 0:
    import loo_reference as lr
    t0 = time.perf_counter()
    chain, _ = e.get_history(g1, g2)
    t1 = time.perf_counter()
    X, y = w["design"], w["y"]
    per = []
    for i in range(host_obs):
        t2 = time.perf_counter()
        a = -0.5 * (y[i] - np.tensordot(X[i], chain, axes=([0], [1]))) ** 2 - 0.9189385332046727
        row = lr.column_f64(a)
        per.append((time.perf_counter() - t2) * 1e3)
        assert row["n_tail"] == rec.n_tail[i]
        print(f"            observation {i}: elpd_loo_i differs from the device's by {abs(row['elpd_loo'] - rec.elpd_loo_i[i]):.1e}, "
              f"khat by {abs(row['pareto_k'] - rec.pareto_k[i]):.1e}")
    print(f"host route: get_history ({chain.nbytes / 1e6:.0f} MB)                {(t1 - t0) * 1e3:10.2f} ms")
    print(f"            NumPy restatement per observation      {fmt(per)}   ({host_obs} observations timed)")
    print(f"            scaled to {nobs} observations            {(t1 - t0) * 1e3 + statistics.median(per) * nobs:10.1f} ms "
          f"= {((t1 - t0) * 1e3 + statistics.median(per) * nobs) / statistics.median(whole):.1f} x HipEngine.loo")
e.close()
