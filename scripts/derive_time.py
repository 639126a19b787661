"""What a derived history costs at C2's shape with a long history (MvNormal d = 5, N = 1024, K = 10, 20 000 generations kept on the
device), m = 2: a variance from a log-variance and one contrast, then their quantiles.

  1. HipEngine.derive                      derive_kernel (demcz_kernels_derive.h), two programs:
                                           "summary"  exp(x[0]) and x[1] - x[2]: the compiler drops the loads of what the function
                                                      never uses (x[3], x[4], logp), so 3 columns are read and 2 written per draw
                                           "all"      every column read: (d + 1 + m) * 8 bytes per draw, the kernel's nominal traffic
  2. ... + DerivedHistory.quantiles        the same result as the host route below, nothing leaves the device
  3. the host route the library offered before: get_history (chain and log_obj), the NumPy restatement of the program,
     quantile_chain on the result (which uploads it again)

The engine runs on a stream made here, so that HIP events can be recorded on it around each derive call: the event time covers the
call's host work between the two records (cache look-ups, buffers from the library's pool) besides the kernel, i.e. it is an upper
bound of the kernel's time; the bandwidth figure is computed from it and is a lower bound.  The wall clock around the same call
(which ends with the stream synchronised) is printed beside it.  Three warm-up calls first (the first compiles the program), then
`reps` timed ones: median and min .. max.  The host route is timed `host_reps` times, parts separately (0: left out, for a run under a profiler).

    python scripts/derive_time.py [reps] [host_reps] [generations]      -> profiles/r11_derive_time.txt
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
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
G = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
d, N, K, m = 5, 1024, 10, 2
PROBS = (0.025, 0.5, 0.975)
HBM_PEAK = 8.0e12                 # bytes/s: the figure DESIGN.md prices every kernel against

SOURCE = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = exp(x[0]);           // a variance from a log-variance
    out[1] = x[1] - x[2];         // a contrast
}
"""
SOURCE_ALL = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    double s = x[0];
    for (int p = 1; p < DEMCZ_D; ++p) s = s + x[p];
    out[0] = s;
    out[1] = logp;
}
"""
# (name, source, columns the compiled kernel loads per draw: global_load_dwordx2 instructions of its loop)
PROGRAMS = (("summary", SOURCE, 3), ("all", SOURCE_ALL, d + 1))


def restatement(chain):
    out = np.empty((chain.shape[0], m, chain.shape[2]), order="F")
    out[:, 0, :] = np.exp(chain[:, 0, :])
    out[:, 1, :] = chain[:, 1, :] - chain[:, 2, :]
    return out


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


w = demc.workloads.mvnormal_problem(d, N)
M0 = w["Zinit"].shape[0]
e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)], eps_scale=w["eps_scale"], seed=1,
                   target=w["target"], stream=stream)
e.set_state(w["Zinit"][-N:], None, w["Zinit"])
e.run(1, G, w["gamma"])
e.synchronize()
draws = N * G
print(f"C2 shape: MvNormal d={d}, N={N}, K={K}, {G} generations on the device; m={m}; {draws} draws; {reps} timed calls after three "
      f"calls; us: median (min .. max)")
for name, source, loads in PROGRAMS:
    p = demc.DerivedProgram(source, d, m)
    t0 = time.perf_counter()
    e.derive(p, 1, G).close()
    first = (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        e.derive(p, 1, G).close()
    nbytes = draws * (loads + m) * 8
    ev_us, wall_us = [], []
    for _ in range(reps):
        hipchk(hip.hipEventRecord(ev0, stream))
        t0 = time.perf_counter()
        h = e.derive(p, 1, G)
        wall_us.append((time.perf_counter() - t0) * 1e6)
        hipchk(hip.hipEventRecord(ev1, stream))
        hipchk(hip.hipEventSynchronize(ev1))
        ms = C.c_float()
        hipchk(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
        ev_us.append(ms.value * 1e3)
        h.close()
    med = statistics.median(ev_us)
    print(f"program '{name}': {loads} columns read + {m} written = {nbytes / 1e9:.3f} GB; first call (compiles) {first:.1f} ms")
    print(f"  HipEngine.derive, HIP events around the call   {fmt(ev_us)}")
    print(f"  HipEngine.derive, wall clock                   {fmt(wall_us)}")
    print(f"  achieved (events, median): {nbytes / med / 1e3:.1f} GB/s = {nbytes / (med * 1e-6) / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak "
          f"(a lower bound: the events also cover the call's host work)")

prog = demc.DerivedProgram(SOURCE, d, m, names=["variance", "contrast"])
both_us, q_us = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    h = e.derive(prog, 1, G)
    t1 = time.perf_counter()
    qd = h.quantiles(1, G, PROBS)
    t2 = time.perf_counter()
    h.close()
    both_us.append((t2 - t0) * 1e6)
    q_us.append((t2 - t1) * 1e6)
print(f"  derive + quantiles on the derived history      {fmt(both_us)}   (quantiles alone {fmt(q_us)})")

if host_reps > 0:
    dl, rs, qc = [], [], []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        chain, lobj = e.get_history(1, G)
        t1 = time.perf_counter()
        v = restatement(chain)
        t2 = time.perf_counter()
        qh = demc.quantile_chain(v, PROBS)
        t3 = time.perf_counter()
        dl.append((t1 - t0) * 1e3); rs.append((t2 - t1) * 1e3); qc.append((t3 - t2) * 1e3)
    tot = [a + b + c for a, b, c in zip(dl, rs, qc)]
    print(f"  host route, total                              {fmt(tot, 'ms')}")
    print(f"    get_history ({(chain.nbytes + lobj.nbytes) / 1e6:.0f} MB)                         {fmt(dl, 'ms')}")
    print(f"    NumPy restatement                            {fmt(rs, 'ms')}")
    print(f"    quantile_chain (uploads {v.nbytes / 1e6:.0f} MB)                 {fmt(qc, 'ms')}")
    print(f"  host route / (derive + quantiles): {statistics.median(tot) * 1e3 / statistics.median(both_us):.1f} x")
    rel = np.max(np.abs(qd - qh) / np.abs(qh))
    print(f"  quantiles of the two routes: max relative difference {rel:.2e} (the contrast's row: {np.max(np.abs(qd[1] - qh[1])):.1e} absolute; "
          f"exp on the device against NumPy's in the other)")
e.close()
