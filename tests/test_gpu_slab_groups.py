"""GPU: demcz_run_checked with nothing decided per slab (threshold <= 0) runs consecutive autostop slabs as one demcz_run call --
one LIVE launch over several slabs where the record span allows (demcz_slab_plan.h) -- and their split-R-hat checks as one batch
(blockIdx.z of the R-hat kernels is the slab).  Everything here is compared with the host loop (demcz_run + demcz_rhat per slab)
or with the oracle, bit for bit; the launch counts tell the grouped path from the per-slab one."""
import os

import numpy as np
import pytest

from helpers import SPLIT_WAVE, oracle_sample

pytestmark = pytest.mark.gpu

THREADS = max(1, min(len(os.sched_getaffinity(0)), 8))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")


def _engine(demc, w, N, d, K, G, seed, lanes=0, Mcap=None):
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=K, Mcap=Mcap or M0 + N * (G // K + 1), Gcap=G, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=seed, target=w["target"], lanes_per_chain=lanes)
    e.set_state(w["Zinit"][-N:], None, w["Zinit"])
    return e


def _max(r):
    return np.nan if np.isnan(r).any() else r.max()


def _host_loop(e, G, every, gamma):
    """The driver loop on the host: demcz_run per slab, demcz_rhat behind it."""
    vecs = []
    for g in range(1, G + 1, every):
        nxt = min(G, g + every - 1)
        e.run(g, nxt, gamma)
        if nxt % every == 0:
            vecs.append(e.rhat(nxt - every + 1, nxt))
    return vecs


def _state(e, G):
    ch, lo = e.get_history(1, G)
    X, lp, Z, M = e.get_state()
    return dict(chain=ch, log_obj=lo, X=X, logp=lp, Z=Z, M=M)


def _same(a, b):
    for k in ("chain", "log_obj", "X", "logp", "Z"):
        assert np.array_equal(a[k], b[k]), k
    assert a["M"] == b["M"]


@pytest.mark.parametrize("d", [2, 5])
def test_grouped_call_equals_the_host_loop(demc, d):
    N, K, every, G, seed = 256, 10, 100, 1200, 91
    w = demc.workloads.mvnormal_problem(d, N)
    a = _engine(demc, w, N, d, K, G, seed)
    a.set_kernel_timing(True)
    g_stop, trace, last = a.run_checked(1, G, w["gamma"], every, 0.0)
    launches = a.info()["window_launches"]
    timed, total_ms = a.get_kernel_time()
    st, du = a.get_kernel_time_series()
    sa = _state(a, G)
    a.close()
    b = _engine(demc, w, N, d, K, G, seed)
    vecs = _host_loop(b, G, every, w["gamma"])
    sb = _state(b, G)
    b.close()
    assert g_stop == G and len(trace) == len(vecs) == G // every
    assert np.array_equal(trace, np.array([_max(v) for v in vecs]), equal_nan=True)
    assert np.array_equal(last, vecs[-1], equal_nan=True)
    _same(sa, sb)
    assert launches < G // every, launches
    assert timed == launches
    # one entry per slab, equal shares of their launch's bracket: means, not events
    assert len(st) == len(du) == G // every
    assert np.isclose(du.sum(), total_ms, rtol=1e-9, atol=0.0)
    assert (np.diff(st) > 0).all() and (du > 0).all()


@pytest.mark.parametrize("N", [1024, 2048])
def test_one_run_across_the_old_cap(demc, oracle, N):
    """A plain demcz_run of 2400 generations, more than two record buffers' worth (64 MiB per buffer, 128 two-chain: 1170
    generations): three launches at the most, every one of them the steady-state kernel's, the buffers sized by arena_span."""
    d, K, G, seed = 5, 10, 2400, 300 + N
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, K, G, seed)
    e.run(1, G, w["gamma"])
    e.synchronize()
    launches, counts, live = e.info()["window_launches"], e.kernel_counts(), e.live_status()
    name = e.kernel_name().split("<")[0]
    s = _state(e, G)
    e.close()
    assert launches <= 3 and counts["ps2"] == launches and counts["ps_general"] == 0 and counts["other"] == 0, (launches, counts)
    assert live == (True, 0)
    assert name == ("demcz::window_kernel_ps2d" if N > 1024 else "demcz::window_kernel_ps2"), name
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, None, w["eps_scale"], w["gamma"], seed, threads=THREADS)
    _same(s, ref)


def test_arena_beside_a_large_archive(demc, oracle):
    """An archive of about 3.3 GB: the record buffers take what is left below the 32-bit reach, the handle keeps its arena and
    with it the steady-state kernel."""
    N, d, K, G, seed = 64, 5, 10, 100, 17
    w = demc.workloads.mvnormal_problem(d, N)
    Mcap = int(3.3e9) // 64                # (d = 5: rows of 64 bytes)
    e = _engine(demc, w, N, d, K, G, seed, Mcap=Mcap)
    e.run(1, G, w["gamma"])
    e.synchronize()
    counts, launches = e.kernel_counts(), e.info()["window_launches"]
    s = _state(e, G)
    e.close()
    assert counts["ps2"] == launches >= 1 and counts["ps_general"] == 0, counts
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, None, w["eps_scale"], w["gamma"], seed)
    _same(s, ref)


@pytest.mark.parametrize("N,d,every,slabs", [(5, 1, 4, 9), (100, 5, 7, 6), (256, 5, 100, 4), (64, 3, 1000, 4)])
def test_batched_check_equals_demcz_rhat(demc, N, d, every, slabs):
    """An odd window (n = 3 of 7), a single chunk, 15 chunks; more than one slab per group in each; a call that ends inside a slab."""
    K, seed = 10, 7
    G = every * slabs + every // 2
    w = demc.workloads.mvnormal_problem(d, N)
    e = _engine(demc, w, N, d, K, G, seed)
    g_stop, trace, last = e.run_checked(1, G, w["gamma"], every, 0.0)
    launches = e.info()["window_launches"]
    vecs = [e.rhat(i * every + 1, (i + 1) * every) for i in range(slabs)]
    lanes = e.info()["lanes_per_chain"]
    e.close()
    assert g_stop == G and len(trace) == slabs
    assert np.array_equal(trace, np.array([_max(v) for v in vecs]), equal_nan=True)
    assert np.array_equal(last, vecs[-1], equal_nan=True)
    if lanes == SPLIT_WAVE and every * slabs <= 1000:
        assert launches < slabs + 1, launches           # (the groups are fewer launches than the slabs; + 1: the partial slab)


def test_timeout_inside_a_grouped_launch(demc, oracle):
    """The debug hook ends a group in front of its generation, so that a launch starts there -- one that spans slabs 3 and 4, and
    times out (the library's software time-out: the kernel returns with an error word, the call is redone)."""
    N, d, K, every, seed = 512, 5, 10, 200, 29
    G = 6 * every
    w = demc.workloads.mvnormal_problem(d, N)
    a = _engine(demc, w, N, d, K, G, seed, SPLIT_WAVE)
    a.debug_set_live_fault(1, 2 * every + 1)
    a.set_live_rearms(0)
    g_stop, trace, last = a.run_checked(1, G, w["gamma"], every, 0.0)
    on, redos = a.live_status()
    launches = a.info()["window_launches"]
    sa = _state(a, G)
    a.close()
    assert redos == 1 and not on
    # first attempt: slabs 1-2, slabs 3-4 (the launch that timed out), slab 5, slab 6, + a cold start; the redo: one launch per
    # K-window
    first = launches - G // K
    assert 4 <= first <= 5, (launches, first)
    b = _engine(demc, w, N, d, K, G, seed, SPLIT_WAVE)
    gb, tb, lb = b.run_checked(1, G, w["gamma"], every, 0.0)
    assert b.live_status() == (True, 0)
    sb = _state(b, G)
    b.close()
    assert g_stop == gb == G and np.array_equal(trace, tb) and np.array_equal(last, lb)
    _same(sa, sb)
    ref = oracle_sample(oracle, w["target"], w["Zinit"], N, K, G, None, w["eps_scale"], w["gamma"], seed)
    _same(sa, ref)
