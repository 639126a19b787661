"""Program targets (DEMCZ_TARGET_PROGRAM, demcz_set_program): what compiling the log-density at run time costs and buys.
  overhead   a program restating MvNormal d = 5 / the isotropic quadratic d = 10 against the built-in target forced to one lane
             per chain (both window_kernel<T, D, true>): kernel time per launch (one K-window, K = 10) at N = 1024, 16384, 131072
  closure    Rosenbrock d = 5 (no built-in target) at C2's shape (N = 1024, K = 10): the program on the device against the
             host-closure pipelined mode (demcz_closure_buffers) with a vectorised NumPy closure -- updates/s
  compile    wall time of the first demcz_set_program of a program (hipRTC) and of a second handle's (the process-wide cache)
usage: python scripts/program_time.py [launches]    (one JSON object; profiles/r06_program_time.txt)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import demc_jl_amd as demc                                  # noqa: E402
from test_gpu_program_target import ISO, MVN, ROSENBROCK    # noqa: E402  (the restatements the GPU tests check bit for bit)

LAUNCHES = int(sys.argv[1]) if len(sys.argv) > 1 else 50
K = 10


def mvn_program(t):
    wp = np.concatenate([np.asarray(t.W)[i, :i + 1] for i in range(t.d)])
    return demc.ProgramTarget(MVN, t.d, data=np.concatenate([t.mu, wp, [t.c0]]))


def per_launch_us(target, w, N, launches):
    d = w["d"]
    Z0 = np.asfortranarray(w["Zinit"])           # (M0 = max(10 d, N) rows)
    G = K * launches
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Z0.shape[0] + N * (G // K + 2), Gcap=0, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=1, target=target, lanes_per_chain=1)
    try:
        e.set_state(Z0[-N:], None, Z0)
        e.run(1, K, w["gamma"])                         # warm-up launch (module load, first touch)
        e.synchronize()
        e.set_kernel_timing(True)
        for g in range(K + 1, K + G + 1, K):            # one demcz_run per K-window: every launch in a bracket of its own
            e.run(g, g + K - 1, w["gamma"])
        n, ms = e.get_kernel_time()
        name = e.kernel_name()
    finally:
        e.close()
    return 1e3 * ms / n, name


def overhead_rows(launches):
    rows = []
    for kind, d in (("mvnormal", 5), ("iso_quad", 10)):
        for N in (1024, 16384, 131072):
            w = demc.workloads.mvnormal_problem(d, N) if kind == "mvnormal" else demc.workloads.iso_quad_problem(d, N)
            prog = mvn_program(w["target"]) if kind == "mvnormal" else demc.ProgramTarget(ISO, d, data=w["mu"])
            b_us, b_name = per_launch_us(w["target"], w, N, launches)
            p_us, p_name = per_launch_us(prog, w, N, launches)
            rows.append(dict(target=kind, d=d, N=N, builtin_us=round(b_us, 2), program_us=round(p_us, 2),
                             ratio=round(p_us / b_us, 4), builtin_kernel=b_name, program_kernel=p_name))
    return rows


def rosen_closure(X):
    """Rosenbrock over the rows of X, vectorised (NumPy)."""
    a = X[:, 1:] - X[:, :-1] * X[:, :-1]
    b = 1.0 - X[:, :-1]
    return -np.sum(100.0 * (a * a) + b * b, axis=1)


def closure_row(gens=300):
    N, d = 1024, 5
    r = np.random.default_rng(5)
    Z0 = np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5)
    eps, gamma = 1e-3 * np.ones(d), 0.8
    M0 = Z0.shape[0]
    out = dict(workload=f"Rosenbrock d={d}, N={N}, K={K}", generations_timed=gens)
    # host closure, pipelined (bench.py configs.closure's fast mode)
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (2 * gens // K + 2), Gcap=2 * gens, blockindex=[range(d)], eps_scale=eps,
                       seed=1, target=rosen_closure)
    try:
        X0 = np.asfortranarray(Z0[-N:])
        e.set_state(X0, rosen_closure(X0), Z0)
        bufs = e.closure_buffers()
        for g in range(1, 2 * gens + 1):
            if g == gens + 1:
                e.synchronize()
                t0 = time.perf_counter()
            Xp = e.propose(g, 0, gamma)
            bufs[1][:] = rosen_closure(Xp)
            e.accept_commit(None)
            e.end_generation(g)
        e.synchronize()
        t_clo = time.perf_counter() - t0
    finally:
        e.close()
    # the program, one launch per K-window, no host step per generation
    gp = 10 * gens
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=M0 + N * (2 * gp // K + 2), Gcap=2 * gp, blockindex=[range(d)], eps_scale=eps, seed=1,
                       target=demc.ProgramTarget(ROSENBROCK, d))
    try:
        e.set_state(Z0[-N:], None, Z0)
        e.run(1, gp, gamma)
        e.synchronize()
        t0 = time.perf_counter()
        e.run(gp + 1, 2 * gp, gamma)
        e.synchronize()
        t_prog = time.perf_counter() - t0
        name = e.kernel_name()
    finally:
        e.close()
    out.update(closure_updates_per_s=N * gens / t_clo, program_updates_per_s=N * gp / t_prog,
               speedup=(N * gp / t_prog) / (N * gens / t_clo), program_kernel=name)
    return out


def compile_row():
    """A program no other part of this process has compiled (a unique constant), then a second handle with the same one."""
    src = ROSENBROCK.replace("100.0", "100.0 + 0.0 * %d.0" % (time.time_ns() % 1000003))
    d, N = 5, 64
    Z0 = np.asfortranarray(np.random.default_rng(0).standard_normal((100, d)))
    mk = lambda target: demc.HipEngine(N=N, d=d, K=K, Mcap=200, Gcap=0, blockindex=[range(d)], eps_scale=1e-3 * np.ones(d),
                                       seed=1, target=target)
    builtin = demc.workloads.mvnormal_problem(d, N)["target"]
    mk(builtin).close()                                 # (the runtime's own start-up is not the compile's)
    t0 = time.perf_counter()
    mk(builtin).close()
    create_s = time.perf_counter() - t0
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        e = mk(demc.ProgramTarget(src, d))
        walls.append(time.perf_counter() - t0)
        e.set_state(Z0[-N:], None, Z0)
        e.close()
    return dict(first_handle_s=round(walls[0], 4), second_handle_s=round(walls[1], 4), builtin_create_s=round(create_s, 4),
                first_set_program_s=round(walls[0] - create_s, 4), second_set_program_s=round(walls[1] - create_s, 4))


if __name__ == "__main__":
    res = dict(compile=compile_row(), overhead=overhead_rows(LAUNCHES), closure=closure_row())
    print(json.dumps(res, indent=1))
