"""What the marginal likelihood by bridge sampling costs on the device: the regression workload (d = 10, N = 1024, nobs = 1000,
built-in target), one 1000-generation slab resident after `burn` slabs of burn-in: 500 generations fit the proposal, the other
500 (512 000 draws) are iterated against 512 000 fresh draws of it.

  1. HipEngine.bridge end to end (demcz_bridge: demcz_mean_cov, the factor on the host, demcz_bridge_posterior,
     demcz_bridge_proposal, demcz_bridge_iterate, demcz_ess of f2), wall clock, with neff given and with neff = "auto" (one more
     demcz_ess, of the parameters)
  2. its layers as calls of their own, wall clock: mean_cov, bridge_posterior, bridge_proposal, bridge_iterate (with f2), ess of f2
     (the kernels themselves: a run of this script under `rocprofv3 --kernel-trace --stats`, summarised by `--trace-summary`)
  3. the host route: get_history of chain and log_obj, then the float64 restatement of tests/bridge_reference.py with the target
     restated in NumPy (a1, the proposal's draws from NumPy's generator, a2, iterate_f64; ESS(f2) left out)

The regression's log_obj is -SSE / 2 with a flat prior, so log Z is known: -SSE_min / 2 + d/2 log 2 pi - 1/2 log det X'X.

Three warm-up calls, then `reps` timed ones: median and min .. max, clocks as found.

    python scripts/bridge_time.py [reps] [host_reps] [burn]             -> profiles/bridge_time.txt
    python scripts/bridge_time.py --trace-summary KERNEL_STATS.csv      kernel totals of a profiled run
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
sys.path.insert(0, str(ROOT / "oracle"))

KERNELS = ("bridge_posterior_kernel", "bridge_proposal_kernel", "bridge_rho0_kernel", "bridge_sum_kernel", "bridge_finish_kernel")


def trace_summary(path):
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    total_key = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls_key = next(k for k in rows[0] if k.lower() == "calls")
    grand = 0.0
    for kn in KERNELS:
        hit = [r for r in rows if kn in r[name_key]]
        ns = sum(float(r[total_key]) for r in hit)
        calls = sum(int(r[calls_key]) for r in hit)
        grand += ns
        print(f"    {kn:26s} n={calls:6d}  total {ns / 1e6:10.3f} ms   {ns / 1e3 / max(calls, 1):9.2f} us each")
    print(f"  the five bridge kernels      {grand / 1e6:10.3f} ms")
    rest = [r for r in rows if not any(kn in r[name_key] for kn in KERNELS) and "window_kernel" not in r[name_key] and "produce" not in r[name_key]]
    rest.sort(key=lambda r: -float(r[total_key]))
    print("  the other kernels of the run (mean_cov, ess; the window kernels and producers of the burn-in left out), largest first:")
    for r in rest[:8]:
        print(f"    {r[name_key][:60]:60s} n={int(r[calls_key]):6d}  total {float(r[total_key]) / 1e6:10.3f} ms")


if len(sys.argv) > 2 and sys.argv[1] == "--trace-summary":
    trace_summary(sys.argv[2])
    sys.exit(0)

import demc_jl_amd as demc                                           # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
burn = int(sys.argv[3]) if len(sys.argv) > 3 else 10
d, N, K, G, nobs = 10, 1024, 10, 1000, 1000


def fmt(ts, unit="ms"):
    return f"{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f}) {unit}"


def timed(fn, n):
    out, r = [], None
    for i in range(3 + n):
        t0 = time.perf_counter()
        r = fn()
        if i >= 3:
            out.append((time.perf_counter() - t0) * 1e3)
    return out, r


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
gh = g1 + G // 2
X, y = w["design"], w["y"]
beta = np.linalg.solve(X.T @ X, X.T @ y)
exact = -0.5 * float(((y - X @ beta) ** 2).sum()) + 0.5 * d * 1.8378770664093453 - 0.5 * float(np.linalg.slogdet(X.T @ X)[1])
print(f"regression workload d={d}, N={N}, K={K}, nobs={nobs}, generations {g1}..{g2} on the device: {gh - g1} generations fit the proposal, "
      f"{N * (g2 - gh + 1)} + {N * (g2 - gh + 1)} draws; {reps} timed calls after three calls; median (min .. max)")
neff = float(np.median(e.ess(gh, g2).ess))
whole, r = timed(lambda: e.bridge(g1, g2, neff=neff), reps)
print(f"HipEngine.bridge end to end, neff given            {fmt(whole)}")
auto, ra = timed(lambda: e.bridge(g1, g2), reps)
print(f"HipEngine.bridge end to end, neff = \"auto\"         {fmt(auto)}")
assert ra.logml == r.logml
print(f"  logml {r.logml:.4f} (exact {exact:.4f}; miss {abs(r.logml - exact) / r.se_logml:.2f} se), se_logml {r.se_logml:.5f}, {r.iterations} updates, "
      f"converged {r.converged}, neff {r.neff:.0f} of {r.n_post}, ESS(f2) {r.ess_f2:.0f}, n_nan {r.n_nan}")
t_mc, _ = timed(lambda: e.mean_cov(g1, gh - 1), reps)
print(f"  mean_cov of the fit window                       {fmt(t_mc)}")


def posterior():
    e.bridge_posterior(gh, g2, r.mean, r.L).close()


def proposal():
    e.bridge_proposal(N, g2 - gh + 1, r.mean, r.L).close()


t_po, _ = timed(posterior, reps)
print(f"  bridge_posterior ({N * (g2 - gh + 1)} draws)                 {fmt(t_po)}")
t_pr, _ = timed(proposal, reps)
print(f"  bridge_proposal  ({N * (g2 - gh + 1)} draws, {nobs} observations each) {fmt(t_pr)}")
post, prop = e.bridge_posterior(gh, g2, r.mean, r.L), e.bridge_proposal(N, g2 - gh + 1, r.mean, r.L)


def iterate():
    it = demc.bridge_iterate(post, prop, neff=neff, want_f2=True)
    it.f2.close()
    return it


t_it, it = timed(iterate, reps)
print(f"  bridge_iterate with f2 ({it.iterations} updates and the moments) {fmt(t_it)}")
assert it.logml == r.logml
f2 = demc.bridge_iterate(post, prop, neff=neff, want_f2=True).f2
t_es, _ = timed(lambda: f2.ess(gh, g2), reps)
print(f"  ess of f2                                        {fmt(t_es)}")
f2.close()
post.close()
prop.close()

if host_reps > 0:
    import bridge_reference as br
    tg, ta, tp, ti = [], [], [], []
    rng = np.random.default_rng(0)
    for _ in range(host_reps):
        t0 = time.perf_counter()
        chain, log_obj = e.get_history(g1, g2)
        chain, log_obj = np.array(chain), np.array(log_obj)
        t1 = time.perf_counter()
        h = G // 2
        a1 = br.posterior_a1(chain[:, :, h:], log_obj[:, h:], r.mean, r.L, br.fma_plain)
        t2 = time.perf_counter()
        z = np.asfortranarray(rng.standard_normal((N, d, G - h)))
        xs, logg = br.proposal(0, N, G - h, r.mean, r.L, br.fma_plain, z)
        rows = br.rows_of(xs)
        sse = np.empty(rows.shape[0])
        for s0 in range(0, rows.shape[0], 16384):                         # (the whole residual matrix would be 4 GB)
            res = y[None, :] - rows[s0:s0 + 16384] @ X.T
            sse[s0:s0 + 16384] = (res * res).sum(axis=1)
        a2 = (-0.5 * sse).reshape(N, G - h) - logg
        t3 = time.perf_counter()
        hit = br.iterate_f64(a1, a2, neff)
        t4 = time.perf_counter()
        tg.append((t1 - t0) * 1e3); ta.append((t2 - t1) * 1e3); tp.append((t3 - t2) * 1e3); ti.append((t4 - t3) * 1e3)
    tot = [a + b + c + dd for a, b, c, dd in zip(tg, ta, tp, ti)]
    print(f"host route: get_history ({(chain.nbytes + log_obj.nbytes) / 1e6:.0f} MB)            {fmt(tg)}")
    print(f"            a1 in NumPy                            {fmt(ta)}")
    print(f"            draws, the target restated, a2         {fmt(tp)}")
    print(f"            iterate_f64 ({hit['iterations']} updates)                {fmt(ti)}")
    print(f"            together (ESS of f2 left out)          {fmt(tot)} = {statistics.median(tot) / statistics.median(whole):.0f} x HipEngine.bridge")
    print(f"            its logml {hit['logml']:.4f} (other draws of the proposal: differs from the device's by {abs(hit['logml'] - r.logml):.4f})")
e.close()
