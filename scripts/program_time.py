"""Program targets (DEMCZ_TARGET_PROGRAM, demcz_set_program): what compiling the log-density at run time costs and buys.
  overhead   a program restating MvNormal d = 5 / the isotropic quadratic d = 10 against the built-in target forced to one lane
             per chain (both window_kernel<T, D, true>): kernel time per launch (one K-window, K = 10) at N = 1024, 16384, 131072
  closure    Rosenbrock d = 5 (no built-in target) at C2's shape (N = 1024, K = 10): the program on the device against the
             host-closure pipelined mode (demcz_closure_buffers) with a vectorised NumPy closure -- updates/s
  compile    wall time of the first demcz_set_program of a program (hipRTC) and of a second handle's (the process-wide cache)
  wave       (`wave` as first argument; profiles/r07_program_wave_time.txt) the layout as a column: five programs at N = 1024, K = 10 on
             the one-lane layout (one launch per K-window) and on DEMCZ_LAYOUT_PROGRAM_WAVE (LIVE launches of 1000 generations), and
             the built-in target on the wave-per-chain layout where the program restates one -- kernel time per K-window from
             demcz_set_kernel_timing, the handles taking turns in one process; median and min..max over the timed launches.
             DEMCZ_NO_PS2=1 DEMCZ_NO_PW_REG=1 in the environment puts the built-in on the general window_kernel_ps / _pw forms
             (the ones the program is compiled into).  Then first-use compile times of the wave unit at d = 5 and d = 20.
  regs       (`regs` as first argument; needs no GPU) registers, spills, scratch and LDS of the wave unit's kernels for the same five
             programs: each is compiled with demcz_program_check_layout under DEMCZ_PROGRAM_DUMP=<temporary directory> (the library
             then writes every code object it compiles there) and read with scripts/kernel_regs.py
usage: python scripts/program_time.py [launches]    (one JSON object; profiles/r06_program_time.txt)
       python scripts/program_time.py wave [rounds]
       python scripts/program_time.py regs"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import demc_jl_amd as demc                                  # noqa: E402
from test_gpu_program_target import ISO, LOGISTIC, MVN, ROSENBROCK    # noqa: E402  (the restatements the GPU tests check bit for bit)

WAVE_MODE = len(sys.argv) > 1 and sys.argv[1] == "wave"
REGS_MODE = len(sys.argv) > 1 and sys.argv[1] == "regs"
_count = sys.argv[2:] if WAVE_MODE else [] if REGS_MODE else sys.argv[1:]
LAUNCHES = int(_count[0]) if _count else (24 if WAVE_MODE else 50)
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


# ---- the layout as a column (DEMCZ_LAYOUT_PROGRAM_WAVE) ------------------------------------------------------------------------
SLAB = 1000          # generations per LIVE launch of the wave layouts (an autostop slab)


def wave_programs():
    N = 1024
    r = np.random.default_rng(104)
    out = []
    for d in (5, 20):
        w = demc.workloads.mvnormal_problem(d, N)
        out.append((f"MvNormal d={d}", mvn_program(w["target"]), w["target"], w["Zinit"], w["eps_scale"], w["gamma"]))
    w = demc.workloads.iso_quad_problem(10, N)
    out.append(("iso-quad d=10", demc.ProgramTarget(ISO, 10, data=w["mu"]), w["target"], w["Zinit"], w["eps_scale"], w["gamma"]))
    Z = np.asfortranarray(0.5 * r.standard_normal((N, 5)) + 0.5)
    out.append(("Rosenbrock d=5", demc.ProgramTarget(ROSENBROCK, 5), None, Z, 1e-3 * np.ones(5), 0.8))
    # (more chains than a LIVE launch holds: the wave layout's one-launch-per-K-window regime, up to PS_MAX_N)
    Z2 = np.asfortranarray(0.5 * r.standard_normal((2048, 5)) + 0.5)
    out.append(("Rosenbrock d=5 N=2048", demc.ProgramTarget(ROSENBROCK, 5), None, Z2, 1e-3 * np.ones(5), 0.8))
    design = 0.3 * r.standard_normal((200, 4))
    labels = (r.random(200) < 0.5).astype(np.float64)
    out.append(("logistic nobs=200 d=4", demc.ProgramTarget(LOGISTIC, 4, data=np.concatenate([design.ravel(), labels])), None,
                np.asfortranarray(r.standard_normal((N, 4))), 1e-3 * np.ones(4), 1.0))
    return N, out


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median=round(float(np.median(us)), 3), min=round(float(us[0]), 3), max=round(float(us[-1]), 3), n=int(us.size))


def _timed_turns(eng, gens, Z0, N, gamma, rounds):
    """The handles of `eng` take turns: two warm-up launches each, then `rounds` timed ones; us per K-window of every timed launch."""
    pos = {k: 0 for k in eng}
    for e in eng.values():
        e.set_state(Z0[-N:], None, Z0)
    for it in range(rounds + 2):
        if it == 2:
            for e in eng.values():
                e.synchronize()
                e.set_kernel_timing(True)
        for k, e in eng.items():
            e.run(pos[k] + 1, pos[k] + gens[k], gamma)
            pos[k] += gens[k]
            e.synchronize()
    out = {}
    for k, e in eng.items():
        e.get_kernel_time()
        _, du = e.get_kernel_time_series()
        out[k] = dict(us_per_window=_stats(1e3 * du / (gens[k] // K)), kernel=e.kernel_name(),
                      live=e.live_status()[0] if gens[k] > K else None, redos=e.live_status()[1])
    return out


def wave_rows(rounds):
    """Per program: the one-lane and the program-wave handle take turns (A/B in one process order), `rounds` timed launches each.
    One-lane: a launch is one K-window; wave: a launch is SLAB generations = SLAB / K windows.  The built-in target on the
    wave-per-chain layout, where the program restates one, is timed the same way in a handle of its own BEFORE and AFTER that pair
    (a device's LIVE budget goes to the first handle that asks and is held until it is destroyed: beside the program's handle the
    built-in one would run one launch per K-window)."""
    N, progs = wave_programs()
    rows = []
    for name, prog, builtin, Z0, eps, gamma in progs:
        d = prog.d
        Z0 = np.asfortranarray(Z0)
        N = Z0.shape[0]                # (every Zinit here has N rows)
        mk = lambda target, lanes, per: demc.HipEngine(N=N, d=d, K=K, Mcap=Z0.shape[0] + N * ((rounds + 3) * per // K + 2), Gcap=0,
                                                       blockindex=[range(d)], eps_scale=eps, seed=1, target=target, lanes_per_chain=lanes)

        def alone(tag):
            e = mk(builtin, demc.LAYOUT_SPLIT_WAVE, SLAB)
            try:
                return _timed_turns({tag: e}, {tag: SLAB}, Z0, N, gamma, rounds)[tag]
            finally:
                e.close()

        row = dict(program=name, N=N, K=K)
        if builtin is not None:
            row["builtin_wave_before"] = alone("builtin_wave_before")
        eng = {"one_lane": mk(prog, 1, K), "program_wave": mk(prog, demc.LAYOUT_PROGRAM_WAVE, SLAB)}
        try:
            row.update(_timed_turns(eng, {"one_lane": K, "program_wave": SLAB}, Z0, N, gamma, rounds))
        finally:
            for e in eng.values():
                e.close()
        if builtin is not None:
            row["builtin_wave_after"] = alone("builtin_wave_after")
        med = lambda k: row[k]["us_per_window"]["median"]
        row["one_lane_over_wave"] = round(med("one_lane") / med("program_wave"), 2)
        row["wave_updates_per_s"] = round(N * K / (med("program_wave") * 1e-6), 0)
        row["one_lane_updates_per_s"] = round(N * K / (med("one_lane") * 1e-6), 0)
        if builtin is not None:
            # (the ratio only where like is compared with like: both handles of the built-in ran LIVE launches, as the program's did)
            row["builtin_live"] = bool(row["builtin_wave_before"]["live"] and row["builtin_wave_after"]["live"])
            if row["builtin_live"] and row["program_wave"]["live"]:
                row["program_over_builtin"] = round(2.0 * med("program_wave") / (med("builtin_wave_before") + med("builtin_wave_after")), 2)
        rows.append(row)
    return rows


def wave_compile_rows():
    out = []
    for d in (5, 20):
        src = ROSENBROCK.replace("100.0", "100.0 + 0.0 * %d.0" % (time.time_ns() % 1000003))
        Z0 = np.asfortranarray(np.random.default_rng(0).standard_normal((200, d)))
        walls = {}
        for lanes, tag in ((1, "one_lane"), (demc.LAYOUT_PROGRAM_WAVE, "wave")):
            for nth in ("first", "second"):
                t0 = time.perf_counter()
                e = demc.HipEngine(N=64, d=d, K=K, Mcap=400, Gcap=0, blockindex=[range(d)], eps_scale=1e-3 * np.ones(d), seed=1,
                                   target=demc.ProgramTarget(src, d), lanes_per_chain=lanes)
                walls[f"{tag}_{nth}_handle_s"] = round(time.perf_counter() - t0, 4)
                e.set_state(Z0[-64:], None, Z0)
                e.close()
        out.append(dict(d=d, **walls))
    return out


def regs_table():
    import os
    import tempfile
    from kernel_regs import kernel_table
    with tempfile.TemporaryDirectory() as td:
        os.environ["DEMCZ_PROGRAM_DUMP"] = td
        print(f"{'program':24s} {'VGPR':>5} {'SGPR':>5} {'sspill':>6} {'vspill':>6} {'scratch':>7} {'LDS':>7}  kernel")
        for name, prog, *_ in wave_programs()[1]:
            if "N=" in name:
                continue               # (the same program again at another N)
            before = set(Path(td).iterdir())
            prog.check(layout=demc.LAYOUT_PROGRAM_WAVE)
            for co in sorted(set(Path(td).iterdir()) - before):
                for r in sorted(kernel_table(co)):
                    if "window_kernel" in r[0]:
                        print(f"{name:24s} {r[1]:5d} {r[3]:5d} {r[4]:6d} {r[5]:6d} {r[6]:7d} {r[7]:7d}  {r[0].split('(')[0].replace('void ', '')}")


if __name__ == "__main__":
    if REGS_MODE:
        sys.path.insert(0, str(Path(__file__).resolve().parent))
        regs_table()
        sys.exit(0)
    if WAVE_MODE:
        import os
        print(json.dumps(dict(env={k: os.environ[k] for k in ("DEMCZ_NO_PS2", "DEMCZ_NO_PW_REG") if k in os.environ},
                              wave=wave_rows(LAUNCHES), compile=wave_compile_rows()), indent=1))
        sys.exit(0)
    res = dict(compile=compile_row(), overhead=overhead_rows(LAUNCHES), closure=closure_row())
    print(json.dumps(res, indent=1))
