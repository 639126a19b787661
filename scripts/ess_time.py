"""What "mean +- MCSE, ESS, R-hat per parameter" costs on C2 (MvNormal d = 5, N = 1024, K = 10) after one 1000-generation slab
and after the full 25-slab run, three ways over the same window of the resident history:

  1. demcz_rhat                                  (the yardstick: one pass over the window)
  2. demcz_ess                                   (R-hat's pass + the lagged products, lags in batches until every parameter stops)
  3. the host route a user has without it: get_history + NumPy FFT autocovariance of every split chain + the same finisher

Wall clock around each library call (every call ends with the stream synchronised), three warm-up calls, then `reps` timed ones:
median and min .. max.  The host route is timed once per window (its download alone dwarfs the others).  Also printed: the lag
batches the adaptive loop took and what one batch of lags costs (demcz_autocov_sums over the first batch: 128 lags at this shape), from which the kernel's
time per sample per lag tile follows.

    python scripts/ess_time.py [reps] [slabs]      -> profiles/r08_ess_time.txt
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


def lag_batch(n):
    """Lags per launch of demcz_ess (the library's plan, acf_chunks / acf_prepare, restated): 32-lag tiles, four to a launch unless
    four tiles of chunk partials would pass 2^24 doubles."""
    waves = (N * d + 63) // 64
    k = max(1, min(n // 64, (4096 + 8 * waves - 1) // (8 * waves), 64))
    per = ((n + k - 1) // k + 31) // 32 * 32
    tile = 2 * ((n + per - 1) // per) * 32 * N * d
    return 32 * max(1, min(4, (1 << 24) // tile))


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
    """get_history, then per parameter: FFT autocovariance of the 2N split chains (zero-padded to twice the length), summed over
    the chains, and the library's host finisher on those sums."""
    t0 = time.perf_counter()
    chain, _ = e.get_history(a, b)
    t1 = time.perf_counter()
    n, m = (b - a + 1) // 2, 2 * N
    nfft = 1 << (2 * n - 1).bit_length()
    sums, between = np.empty((d, n), order="F"), np.empty(d)
    for p in range(d):
        x = np.concatenate([chain[:, p, :n], chain[:, p, n:2 * n]], axis=0)
        mean = x.mean(axis=1, keepdims=True)
        f = np.fft.rfft(x - mean, nfft, axis=1)
        sums[p] = np.fft.irfft(f * np.conj(f), nfft, axis=1)[:, :n].sum(axis=0)
        between[p] = ((mean - mean.mean()) ** 2).sum()
    out = demc.ess_from_sums(m, n, sums, between)
    t2 = time.perf_counter()
    return out, (t1 - t0) * 1e3, (t2 - t1) * 1e3, chain.nbytes


w = demc.workloads.mvnormal_problem(d, N)
M0 = w["Zinit"].shape[0]
e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=1,
                   target=w["target"])
e.set_state(w["Zinit"][-N:], None, w["Zinit"])
print(f"C2: MvNormal d={d}, N={N}, K={K}; {reps} timed calls after 3 warm-up calls, wall clock in us: median (min .. max)")
done = 0
for upto in sorted({every, G}):
    e.run(done + 1, upto, w["gamma"])
    e.synchronize()
    done = upto
    n = upto // 2
    r = e.ess(1, upto)
    lags = int(np.max(np.where(r.converged == 1, 2 * r.pairs + 2, n)))
    B = lag_batch(n)
    batches = -(-min(lags, n) // B)
    print(f"\nwindow 1..{upto} ({upto // every} slab(s), n = {n} samples per split chain, {2 * N} split chains)")
    print(f"  ess {np.round(r.ess).astype(int).tolist()}  tau {np.round(r.tau, 2).tolist()}  pairs {r.pairs.tolist()}  converged {r.converged.tolist()}")
    print(f"  rhat {np.round(e.rhat(1, upto), 4).tolist()}")
    t_rhat = timed(lambda: e.rhat(1, upto))
    t_ess = timed(lambda: e.ess(1, upto))
    t_one = timed(lambda: e.autocov_sums(1, upto, 0, B - 1))
    print("  demcz_rhat                       %9.1f (%.1f .. %.1f)" % t_rhat)
    print("  demcz_ess                        %9.1f (%.1f .. %.1f)   %d lag batch(es) of %d (lags 0..%d of %d)" % (t_ess + (batches, B, min(B * batches, n) - 1, n - 1)))
    print("  demcz_autocov_sums, one batch    %9.1f (%.1f .. %.1f)   lags 0..%d, incl. R-hat's moments pass" % (t_one + (B - 1,)))
    per = (t_one[0] - t_rhat[0]) * 1e-6 / (N * d * 2 * n * (B // 32))
    print(f"    -> {per * 1e12:.2f} ps per sample per 32-lag tile beyond the moments pass; rhat_moments_kernel's pass with its reductions and "
          f"copy: {t_rhat[0] * 1e-6 / (N * d * 2 * n) * 1e12:.2f} ps per sample")
    h, t_dl, t_np, nbytes = host_route(e, 1, upto)
    same = np.array_equal(h.pairs, r.pairs) and np.array_equal(h.converged, r.converged)
    print(f"  host route                       {(t_dl + t_np) * 1e3:9.1f}   = get_history {t_dl:.1f} ms ({nbytes / 1e6:.0f} MB) + NumPy FFT autocovariance {t_np:.1f} ms;"
          f" pairs / converged {'equal to' if same else 'DIFFER from'} the device's, max |tau - tau_device| = {np.max(np.abs(h.tau - r.tau)):.2e}")
e.close()
