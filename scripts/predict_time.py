"""What posterior predictive draws cost on the device.

  1. C2's shape with a long history (MvNormal d = 5, N = 1024, K = 10, 20 000 generations kept on the device), m = 2:
       HipEngine.predict   two normals a draw (one Philox block, one Box-Muller pair) added to a sum of all columns and to logp
       HipEngine.derive    the same function without the normals: derive_kernel, the traffic floor -- every column read,
                           (d + 1 + m) * 8 bytes a draw
     and their ratio.
  2. The regression example of the README: y_i ~ N(a + b t_i, sigma), nobs = 1000, x = (a, b, log sigma); over a window of 1000
     generations of N = 1024 chains a whole y_rep is drawn per posterior draw and two realised discrepancies are compared with the
     data's: chi^2 = sum ((y - mu) / sigma)^2 and max |y - mu| / sigma.
       HipEngine.ppc       everything on the device, six counters come back
       the host route      get_history, numpy.random.Generator.standard_normal, the two statistics in NumPy, in slices of 10
                           generations (a whole window of y_rep is 8 GB)
     The history is a stand-in (an MvNormal posterior around the generating values): neither route's cost depends on the values.

The engine runs on a stream made here, so that HIP events can be recorded on it around each call: the event time covers the call's
host work between the two records besides the kernel, i.e. it is an upper bound of the kernel's time.  Three warm-up calls first
(the first compiles the program), then `reps` timed ones: median and min .. max.

    python scripts/predict_time.py [reps] [host_reps] [generations]      -> profiles/predict_time.txt
"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import demc_jl_amd as demc                                           # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
G = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
d, N, K, m = 5, 1024, 10, 2
HBM_PEAK = 8.0e12                 # bytes/s: the figure DESIGN.md prices every kernel against

PREDICT = """
__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out)
{
    double s = x[0];
    for (int p = 1; p < DEMCZ_D; ++p) s = s + x[p];
    out[0] = s + demcz_normal(rng);
    out[1] = logp + demcz_normal(rng);
}
"""
DERIVE = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    double s = x[0];
    for (int p = 1; p < DEMCZ_D; ++p) s = s + x[p];
    out[0] = s;
    out[1] = logp;
}
"""
# The README's example.  data: t[0..NOBS), then y[0..NOBS).  Both columns are differences of a realised discrepancy between the
# replicate and the data at the same draw, to be compared with 0.
NOBS = 1000
REGRESSION = """
__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out)
{
    const double a = x[0], b = x[1], sigma = exp(x[2]);
    double chi_rep = 0.0, chi_obs = 0.0, max_rep = 0.0, max_obs = 0.0;
    for (int i = 0; i < NOBS; ++i) {
        const double mu = a + b * data[i];
        const double z_rep = demcz_normal(rng);                 // (y_rep - mu) / sigma
        const double z_obs = (data[NOBS + i] - mu) / sigma;
        chi_rep += z_rep * z_rep;
        chi_obs += z_obs * z_obs;
        max_rep = fmax(max_rep, fabs(z_rep));
        max_obs = fmax(max_obs, fabs(z_obs));
    }
    out[0] = chi_rep - chi_obs;
    out[1] = max_rep - max_obs;
}
"""

hip = C.CDLL("libamdhip64.so")


def hipchk(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
hipchk(hip.hipStreamCreateWithFlags(C.byref(stream), 1))             # hipStreamNonBlocking
hipchk(hip.hipEventCreate(C.byref(ev0)))
hipchk(hip.hipEventCreate(C.byref(ev1)))


def fmt(ts, unit="us"):
    return f"{statistics.median(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f}) {unit}"


def timed(call, close=True):
    """Three warm-up calls (the first one's wall time in ms is returned), then `reps` timed: event and wall times in us."""
    t0 = time.perf_counter()
    r = call()
    first = (time.perf_counter() - t0) * 1e3
    if close:
        r.close()
    for _ in range(2):
        r = call()
        if close:
            r.close()
    ev_us, wall_us = [], []
    for _ in range(reps):
        hipchk(hip.hipEventRecord(ev0, stream))
        t0 = time.perf_counter()
        r = call()
        wall_us.append((time.perf_counter() - t0) * 1e6)
        hipchk(hip.hipEventRecord(ev1, stream))
        hipchk(hip.hipEventSynchronize(ev1))
        ms = C.c_float()
        hipchk(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
        ev_us.append(ms.value * 1e3)
        if close:
            r.close()
    return first, ev_us, wall_us, r


def engine(w, dd, gens, seed):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=dd, K=K, Mcap=M0 + N * (gens // K + 1), Gcap=gens, blockindex=[range(dd)], eps_scale=w["eps_scale"],
                       seed=seed, target=w["target"], stream=stream)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    e.run(1, gens, w["gamma"])
    e.synchronize()
    return e


# ---- 1. C2's shape -----------------------------------------------------------------------------------------------------------
e = engine(demc.workloads.mvnormal_problem(d, N), d, G, seed=1)
draws = N * G
nbytes = draws * (d + 1 + m) * 8
print(f"C2 shape: MvNormal d={d}, N={N}, K={K}, {G} generations on the device; m={m}; {draws} draws; {reps} timed calls after three "
      f"calls; us: median (min .. max)")
print(f"every column read + {m} written = {nbytes / 1e9:.3f} GB")
med = {}
for name, call in (("predict", lambda p=demc.PredictiveProgram(PREDICT, d, m): e.predict(p, 1, G)),
                   ("derive", lambda p=demc.DerivedProgram(DERIVE, d, m): e.derive(p, 1, G))):
    first, ev_us, wall_us, _ = timed(call)
    med[name] = statistics.median(ev_us)
    print(f"HipEngine.{name}: first call (compiles) {first:.1f} ms")
    print(f"  HIP events around the call   {fmt(ev_us)}")
    print(f"  wall clock                   {fmt(wall_us)}")
    print(f"  achieved (events, median): {nbytes / med[name] / 1e3:.1f} GB/s = {nbytes / (med[name] * 1e-6) / HBM_PEAK:.3f} of the "
          f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak (a lower bound: the events also cover the call's host work)")
print(f"predict / derive (events, medians): {med['predict'] / med['derive']:.2f} x; {2 * draws / (med['predict'] * 1e-6) / 1e9:.2f} G normals/s")
e.close()

# ---- 2. the regression example -------------------------------------------------------------------------------------------------
W = 1000
r = np.random.default_rng(7)
t = r.standard_normal(NOBS)
truth = np.array([1.0, 2.0, np.log(0.5)])
y = truth[0] + truth[1] * t + np.exp(truth[2]) * r.standard_normal(NOBS)
post = dict(target=demc.MvNormalTarget(truth, np.diag([2.5e-4, 2.5e-4, 5e-4])), Zinit=np.asfortranarray(truth + 0.02 * r.standard_normal((N, 3))),
            eps_scale=1e-5 * np.ones(3), gamma=2.38)
e = engine(post, 3, W, seed=2)
prog = demc.PredictiveProgram(REGRESSION, 3, 2, data=np.concatenate([t, y]), options=[f"-DNOBS={NOBS}"], names=["chi2", "max"])
normals = N * W * NOBS
print(f"\nregression example: nobs={NOBS}, N={N}, a window of {W} generations: {N * W} replicated data sets, {normals:.3g} normals")
first, ev_us, wall_us, res = timed(lambda: e.ppc(prog, 1, W), close=False)
mev = statistics.median(ev_us)
print(f"HipEngine.ppc, two statistics: first call (compiles) {first:.1f} ms")
print(f"  HIP events around the call   {fmt(ev_us)}")
print(f"  wall clock                   {fmt(wall_us)}")
print(f"  {normals / (mev * 1e-6) / 1e9:.2f} G normals/s (events, median)")
print(f"  p-values {dict(zip(res.names, res.p_value.tolist()))}, nan {res.nan.tolist()}")
if host_reps > 0:
    dl, gen, st = [], [], []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        chain, _ = e.get_history(1, W)
        t1 = time.perf_counter()
        rng = np.random.default_rng(3)
        gt = np.zeros(2, dtype=np.int64)
        tg = ts = 0.0
        for g in range(0, W, 10):
            x = chain[:, :, g:g + 10]
            ta = time.perf_counter()
            z_rep = rng.standard_normal((N, x.shape[2], NOBS))
            tb = time.perf_counter()
            mu = x[:, 0, :, None] + x[:, 1, :, None] * t
            z_obs = (y - mu) / np.exp(x[:, 2, :, None])
            gt[0] += ((z_rep ** 2).sum(axis=2) - (z_obs ** 2).sum(axis=2) >= 0).sum()
            gt[1] += (np.abs(z_rep).max(axis=2) - np.abs(z_obs).max(axis=2) >= 0).sum()
            tg += tb - ta
            ts += time.perf_counter() - tb
        dl.append((t1 - t0) * 1e3); gen.append(tg * 1e3); st.append(ts * 1e3)
    tot = [a + b + c for a, b, c in zip(dl, gen, st)]
    print(f"host route, total                  {fmt(tot, 'ms')}")
    print(f"  get_history ({chain.nbytes / 1e6:.0f} MB)              {fmt(dl, 'ms')}")
    print(f"  Generator.standard_normal        {fmt(gen, 'ms')}   ({normals / (statistics.median(gen) * 1e-3) / 1e9:.2f} G normals/s)")
    print(f"  the two statistics               {fmt(st, 'ms')}")
    print(f"  p-values {(gt / (N * W)).tolist()} (another generator: they agree to Monte Carlo error only)")
    print(f"host route / ppc: {statistics.median(tot) * 1e3 / statistics.median(wall_us):.0f} x")
e.close()
