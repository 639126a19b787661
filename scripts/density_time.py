"""What the posterior densities cost on C2 (MvNormal d = 5, N = 1024, K = 10) over one 1000-generation slab of the resident history
(S = 1 024 000 draws per parameter), each beside the route a user has without it:

  demcz_histogram at 33 and at 4096 bins            get_history + np.histogram per parameter
  demcz_histogram2d, all pairs at 32 x 32           get_history + np.histogram2d per pair
  ... the same at d = 20 on 257 chains, S = 1 024 145 (190 pairs; a history uploaded once and derived on the device)
  demcz_hdi at 0.94                                 get_history + np.sort and the arg-min per parameter
  demcz_quantiles at 2 probabilities                (its counting passes read the bytes the marginal histogram reads)

The automatic range is part of the histogram calls (demcz_quantiles at probabilities 0 and 1: eight counting passes); the rows
"given range" leave it out.  Wall clock around each library call (every call ends with the stream synchronised), three warm-up
calls, then `reps` timed ones: median and min .. max.  The host routes are timed once.  The device's counts and interval ends
are checked against the host's.

    python scripts/density_time.py [reps]      -> profiles/density_time.txt
    rocprofv3 --kernel-trace --stats -- python scripts/density_time.py 3      (per-kernel times -> profiles/density_kernels.txt)
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


def once(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def draws(chain, p):
    return np.ascontiguousarray(chain[:, p, :]).ravel()


def host_hdi(x, prob):
    s = np.sort(x)
    m = min(int(np.floor(prob * s.size)), s.size - 1)
    i = int(np.argmin(s[m:] - s[:s.size - m]))
    return s[i], s[i + m]


def report(name, t, host=None):
    line = "  %-44s %9.2f (%.2f .. %.2f)" % ((name,) + t)
    if host is not None:
        line += "   host route %9.2f   device / host = %.3f" % (host, t[0] / host)
    print(line)


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

(chain, _), t_get = once(lambda: e.get_history(1, G))
rng = np.stack([chain.min(axis=(0, 2)), chain.max(axis=(0, 2))], axis=1)
pairs = [(p, q) for p in range(d) for q in range(p + 1, d)]
print(f"  get_history of the window                    {t_get:9.2f}   ({chain.nbytes / 1e6:.0f} MB; part of every host route below)")

for nb in (33, 4096):
    got = e.histogram(1, G, nb)
    want, t_np = once(lambda: [np.histogram(draws(chain, p), bins=nb, range=tuple(rng[p]))[0] for p in range(d)])
    assert np.array_equal(got.counts, np.array(want)), nb
    report(f"demcz_histogram, {nb} bins", timed(lambda: e.histogram(1, G, nb)), t_get + t_np)
    report(f"demcz_histogram, {nb} bins, given range", timed(lambda: e.histogram(1, G, nb, rng)))

got = e.histogram2d(1, G, None, 32)
want, t_np = once(lambda: [np.histogram2d(draws(chain, p), draws(chain, q), bins=[got.edges[0][p], got.edges[1][q]])[0] for p, q in pairs])
assert np.array_equal(got.counts, np.array(want).astype(np.int64))
report(f"demcz_histogram2d, {len(pairs)} pairs at 32 x 32", timed(lambda: e.histogram2d(1, G, None, 32)), t_get + t_np)
report(f"demcz_histogram2d, {len(pairs)} pairs, given range", timed(lambda: e.histogram2d(1, G, None, 32, rng)))
report("demcz_histogram2d, 1 pair at 128 x 128", timed(lambda: e.histogram2d(1, G, [(0, 1)], 128, rng)))

got = e.hdi(1, G, 0.94)
want, t_np = once(lambda: [host_hdi(draws(chain, p), 0.94) for p in range(d)])
assert np.array_equal(got, np.array(want))
report("demcz_hdi at 0.94", timed(lambda: e.hdi(1, G, 0.94)), t_get + t_np)
report("demcz_hdi at 16 probabilities", timed(lambda: e.hdi(1, G, np.linspace(0.05, 0.95, 16))))
report("demcz_quantiles, 2 probabilities (8 passes)", timed(lambda: e.quantiles(1, G, (0.0, 1.0))))
with e.rank_normalize(1, G, ranks=True) as _h:
    pass
report("demcz_rank_normalize, raw ranks", timed(lambda: e.rank_normalize(1, G, ranks=True).close()))
e.close()

# d = 20 on 257 chains, scaled to the same S: a world made here, uploaded once (the normal scores of a host array are a history on
# the device), 190 pairs
d2, N2 = 20, 257
G2 = -(-S // N2)
gen = np.random.default_rng(1)
A = np.eye(d2) + 0.5 * gen.standard_normal((d2, d2)) / np.sqrt(d2)
world = np.asfortranarray(np.einsum("pq,nqg->npg", A, gen.standard_normal((N2, d2, G2))))
pairs2 = [(p, q) for p in range(d2) for q in range(p + 1, d2)]
print(f"d={d2}, N={N2}, {G2} generations, S = {N2 * G2} draws per parameter ({world.nbytes / 1e6:.0f} MB), {len(pairs2)} pairs")
with demc.rank_normalize_chain(world) as h:
    (z, t_get2) = once(lambda: h.get())
    rng2 = np.stack([z.min(axis=(0, 2)), z.max(axis=(0, 2))], axis=1)
    got = h.histogram2d(1, G2, None, 32)
    want, t_np = once(lambda: [np.histogram2d(draws(z, p), draws(z, q), bins=[got.edges[0][p], got.edges[1][q]])[0] for p, q in pairs2])
    assert np.array_equal(got.counts, np.array(want).astype(np.int64))
    report(f"demcz_histogram2d, {len(pairs2)} pairs at 32 x 32", timed(lambda: h.histogram2d(1, G2, None, 32)), t_get2 + t_np)
    report(f"demcz_histogram2d, {len(pairs2)} pairs, given range", timed(lambda: h.histogram2d(1, G2, None, 32, rng2)))
    report("demcz_histogram, 33 bins", timed(lambda: h.histogram(1, G2, 33)))
    report("demcz_hdi at 0.94", timed(lambda: h.hdi(1, G2, 0.94)))
