"""GPU: replica groups in every hand-off kernel, form and shard shape, bit for bit against the oracle's unsharded run.

tests/peer_cases.py holds the worlds: the single-handle suites' worlds cut into R = 2 or 3 equal shards, one handle each, all in
this process on the one device (demcz_peer_group), every form of the family on each member; shards whose last workgroup is
partly filled; layouts without the hand-off, which run in lockstep from the start; a few named edges.  By the oracle alone
(tests/test_peer_cases.py) every ordered pair of ranks draws rows the other has just appended, and every member appends rows that
are never drawn again.  Every piece is given to every member before any member is asked for anything.  Behind every piece each
member's kernel name and count of window launches are held to the plan; a group with the hand-off must be LIVE on every member
with no redo, behind every piece and at the end (a launch that timed out and was redone in lockstep gives the same numbers and
proves nothing about the hand-off: that fails here, it does not skip).  At the end chain, log_obj, X and logp, concatenated over
the members in rank order, EVERY member's archive and M, and the ballots' changed_total summed over the members (from the first
generation and from the last launch's first) are compared.  No tolerance anywhere.  The poll limit is the
library's default; nothing is forced to time out here (tests/test_gpu_peer.py has those tests)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import peer_cases as pc
from helpers import same_bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def group_run(demc, run):
    """The library over the run's pieces on R grouped handles.  dict: the oracle run's keys over all members (Z, M: per member),
    `names`, `launches`, `live` per piece and member, `peer`, `layouts`, `live_end`, `changed`, `changed_tail`."""
    case, R, n_loc = run["case"], run["R"], run["n_loc"]
    w, N, d, K, G = case["problem"], case["N"], case["d"], case["K"], case["G"]
    M0 = w["Zinit"].shape[0]
    X0 = w["Zinit"][-N:]
    tail_g = pc.plan(run)[1]
    changed_from = run["resume_at"] + 1 if run["resume_at"] else 1       # (demcz_set_state opens the history window anew)
    es = []
    try:
        for r in range(R):
            e = demc.HipEngine(N=n_loc, d=d, K=K, Mcap=M0 + N * (G // K + 1), Gcap=G if run["history"] else 0, blockindex=case["blocks"],
                               eps_scale=w["eps_scale"], seed=case["seed"], target=w["target"], chain_id0=r * n_loc, lanes_per_chain=run["lanes"])
            es.append(e)
            e.set_state(X0[r * n_loc:(r + 1) * n_loc], None, w["Zinit"])
        layouts = [e.info()["lanes_per_chain"] for e in es]
        demc.HipEngine.peer_group(es)
        peer = [e.peer_status() for e in es]
        names, launches, live = [], [], []
        for a, b, tempered, _ in case["pieces"]:
            for e in es:                          # every member is given the call before any member is asked for anything
                e.run(a, b, case["gamma"], case["temperature"][a - 1:b] if tempered else None)
            if not run["handoff"]:
                es[0].synchronize()               # a lockstep group executes what its members have logged at a verification
            names.append([e.kernel_name() for e in es])
            launches.append([e.info()["window_launches"] for e in es])
            live.append([tuple(e.live_status()) for e in es])
            if b == run["resume_at"]:
                states = [e.get_state() for e in es]
                for e, (X, lp, Z, M) in zip(es, states):
                    e.set_state(np.array(X), np.array(lp), np.array(Z[:M]))
        for e in es:
            e.synchronize()
        got = dict(names=names, launches=launches, live=live, peer=peer, layouts=layouts, live_end=[tuple(e.live_status()) for e in es])
        if run["history"]:
            hist = [e.get_history(1, G) for e in es]
            got["chain"] = np.concatenate([h[0] for h in hist], axis=0)
            got["log_obj"] = np.concatenate([h[1] for h in hist], axis=0)
        states = [e.get_state() for e in es]
        got["X"] = np.concatenate([np.array(s[0]) for s in states], axis=0)
        got["logp"] = np.concatenate([np.array(s[1]) for s in states])
        got["Z"] = [np.array(s[2][:s[3]]) for s in states]
        got["M"] = [s[3] for s in states]
        totals = [e.changed_total(changed_from, G, with_source=True) for e in es]
        tails = [e.changed_total(tail_g, G, with_source=True) for e in es]
        got.update(changed=sum(t[0] for t in totals), from_ballots=[t[1] for t in totals], changed_tail=sum(t[0] for t in tails),
                   changed_from=changed_from, tail_g=tail_g)
        return got
    finally:
        for e in es:
            e.close()


def check(demc, oracle, monkeypatch, run):
    for v in run["env"]:
        monkeypatch.setenv(v, "1")                # (read in demcz_create; DEMCZ_MLB_L32 once per process)
    got = group_run(demc, run)
    what, R, case = run["id"], run["R"], run["case"]
    plan, _ = pc.plan(run)
    assert got["layouts"] == [run["layout"]] * R, what
    assert got["peer"] == [(1, R - 1)] * R, what
    status = (True, 0) if run["handoff"] else (False, 0)      # (lockstep-only: demcz_peer_group released every member's LIVE claim)
    for (a, b, _, form), (name, count), ran, n, live in zip(case["pieces"], plan, got["names"], got["launches"], got["live"]):
        assert live == [status] * R, \
            f"{what}, generations {a}..{b}: LIVE status {live} (a hand-off that timed out and was redone in lockstep did not produce these numbers)"
        assert ran == [name] * R, f"{what}, generations {a}..{b} ({form}): planned {name}, ran {ran}"
        assert n == [count] * R, f"{what}, generations {a}..{b}: planned {count} window launches, made {n}"
    assert got["live_end"] == [status] * R, f"{what}: LIVE status at the end {got['live_end']}: a hand-off timed out and the group was redone in lockstep"
    ref = run["ref"](oracle)
    same_bits(got, ref, keys=("chain", "log_obj", "X", "logp") if run["history"] else ("X", "logp"), what=what)
    for r in range(R):                            # every replica is the whole archive
        assert got["M"][r] == ref["M"], f"{what}: member {r} has M = {got['M'][r]}, the oracle {ref['M']}"
        same_bits(dict(Z=got["Z"][r]), ref, keys=("Z",), what=f"{what}: the archive of member {r}")
    g = got["changed_from"]
    assert got["changed"] == int(ref["changed"][g - 1:].sum()), f"{what}: changed_total from generation {g}: {got['changed']} (from the ballots: {got['from_ballots']})"
    g = got["tail_g"]
    assert got["changed_tail"] == int(ref["changed"][g - 1:].sum()), f"{what}: changed_total from generation {g}, the last launch's first: {got['changed_tail']}"
    return got


MAIN, SHAPES, LOCKSTEP, EDGES = pc.main_runs(), pc.shape_runs(), pc.lockstep_runs(), pc.edge_runs()


@pytest.mark.parametrize("run", MAIN, ids=pc.ids(MAIN))
def test_equal_shards_every_form_on_every_member(demc, oracle, monkeypatch, run):
    check(demc, oracle, monkeypatch, run)


@pytest.mark.parametrize("run", SHAPES, ids=pc.ids(SHAPES))
def test_shards_whose_last_workgroup_is_partly_filled(demc, oracle, monkeypatch, run):
    """n_loc = 1, 3, 5, 9, 17 in two shards and 7 in three: shadow chains beside the last chain of every member but the last one's
    are chains of the NEXT member in the archive's rows; a small archive, so that fresh rows are a large share of every draw."""
    check(demc, oracle, monkeypatch, run)


@pytest.mark.parametrize("run", LOCKSTEP, ids=pc.ids(LOCKSTEP))
def test_layouts_without_the_handoff_run_in_lockstep(demc, oracle, monkeypatch, run):
    check(demc, oracle, monkeypatch, run)


@pytest.mark.parametrize("run", EDGES, ids=pc.ids(EDGES))
def test_named_edges(demc, oracle, monkeypatch, run):
    """Gcap = 0 (state, archives and the ballots' totals); a group given its own state back in the middle of a window; zero, tiny
    and huge temperatures."""
    if "zero_temperature" in run["id"]:
        assert {0.0, 1e-300, 1e300} <= set(run["case"]["temperature"].tolist())
    got = check(demc, oracle, monkeypatch, run)
    if not run["history"]:
        assert all(got["from_ballots"]), "Gcap = 0: changed_total has only the ballots to answer from"


# ---- the 32-lane split form: DEMCZ_MLB_L32 is read once per process -----------------------------------------------------------------------
if os.environ.get(pc.L32):
    def test_thirty_two_lanes_in_a_group(demc, oracle, monkeypatch):
        """(Collected only in a process that has the switch: the child of the test below.)"""
        got = check(demc, oracle, monkeypatch, pc.l32_run())
        assert all(n.startswith("demcz::window_kernel_mlb<MVNORMAL, 20, 32, true, true") for ns in got["names"] for n in ns), got["names"]


def test_the_thirty_two_lane_group_in_a_child_process():
    """The one child process of this file: the switch cannot be set in a process that has created a handle before."""
    env = dict(os.environ)
    env[pc.L32] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_peer_forms.py",
                        "-k", "test_thirty_two_lanes_in_a_group"], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
