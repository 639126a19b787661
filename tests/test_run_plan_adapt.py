"""CPU tier of the launch schedule of a handle that adapts its crossover class weights: demcz_run_plan.h's adapt_every / adapt_until /
adapt_after, walked by a stand-alone program (tests/c_abi/run_plan_adapt_main.cpp, built under AddressSanitizer and UBSan like
run_plan_main.cpp) over whole calls of a one-lane handle and compared launch by launch with a Python restatement of the rule; and
the properties the executor relies on whatever the restatement says: the launches tile the call, every update position inside the
call ends a launch that is followed by the update, no other launch is, and a launch lies wholly at or in front of `until` or wholly
behind it (its `accumulate` is one flag)."""
import re
import shutil
import subprocess
from collections import namedtuple
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

Case = namedtuple("Case", "K g_from length E rng_offset snooker every until")
Launch = namedtuple("Launch", "g w_end snooker adapt_after accumulate nbound")


def restated(c):
    """plan_launch for span 0, no split: the K-window (or the batch of E windows), the snooker rule, then the update positions"""
    g_to = c.g_from + c.length - 1
    g, out = c.g_from, []
    while g <= g_to:
        nb = -(-g // c.K) * c.K
        w_end = min(nb, g_to)
        if c.E > 0:
            w_end = min(-(-(nb // c.K) // c.E) * c.E * c.K, g_to)
        snooker = False
        if c.snooker:
            if (g + c.rng_offset) % c.snooker == 0:
                w_end, snooker = g, True
            else:
                w_end = min(w_end, g + (c.snooker - (g + c.rng_offset) % c.snooker) - 1)
        acc = c.every > 0 and g + c.rng_offset <= c.until
        after = False
        if acc:
            u = -(-(g + c.rng_offset) // c.every) * c.every - c.rng_offset
            w_end = min(w_end, u)
            after = w_end == u
        out.append(Launch(g, w_end, int(snooker), int(after), int(acc), w_end // c.K - (g - 1) // c.K))
        g = w_end + 1
    return out


def cases():
    out = []
    K = 10
    out += [Case(K, 1, 100, 0, 0, 0, 7, 70)]               # every coprime to K
    out += [Case(K, 1, 100, 0, 0, 0, 20, 80)]              # a multiple of K
    out += [Case(K, 1, 40, 0, 0, 0, 1, 25)]                # every generation
    out += [Case(K, 1, 60, 0, 0, 4, 12, 48)]               # snooker generations on the update positions
    out += [Case(K, 1, 60, 0, 0, 5, 7, 49)]                # ... and beside them
    out += [Case(K, 15, 30, 0, 0, 0, 14, 42)]              # a call that starts one past an update
    out += [Case(K, 8, 35, 0, 0, 0, 7, 42)]                # ... and one that ends on `until`
    out += [Case(K, 1, 50, 0, 13, 0, 7, 42)]               # a resumed run: positions in the stream numbering
    out += [Case(K, 4, 50, 0, 13, 3, 10, 60)]
    out += [Case(K, 1, 90, 2, 0, 0, 7, 70)]                # append lag: launches over several K-windows are cut as well
    out += [Case(K, 1, 90, 3, 5, 0, 25, 75)]
    out += [Case(K, 50, 30, 0, 0, 0, 7, 42)]               # wholly behind `until`
    out += [Case(K, 1, 30, 0, 0, 0, 0, 0)]                 # off
    # a grid over small numbers
    for Kk in (1, 5, 7):
        for g_from in (1, 2, Kk + 1):
            for length in (1, Kk, 3 * Kk + 2, 40):
                for E in (0, 2):
                    for off in (0, 3):
                        for sn in (0, 3):
                            for every, until in ((1, 4), (3, 9), (5, 20), (8, 8), (11, 33)):
                                out.append(Case(Kk, g_from, length, E, off, sn, every, until))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("run_plan_adapt")
    exe = tmp / "run_plan_adapt_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "c_abi" / "run_plan_adapt_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    (tmp / "cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in CASES))
    p = subprocess.run([str(exe), "walk", str(tmp / "cases.txt")], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    got, cur = [], None
    for line in p.stdout.splitlines():
        if line.startswith("case"):
            cur = []
            got.append(cur)
        else:
            cur.append(Launch(*(int(v) for v in line.split())))
    assert len(got) == len(CASES)
    (tmp / "bad.txt").write_text("10 1 10 0 0 0 7 20\n")          # until is no multiple of every
    assert subprocess.run([str(exe), "walk", str(tmp / "bad.txt")], capture_output=True, text=True).returncode == 2
    return got


def test_every_launch_is_the_restated_one(walked):
    for c, launches in zip(CASES, walked):
        assert launches == restated(c), c


def test_the_named_cases_cut_where_they_should(walked):
    by = dict(zip(CASES, walked))
    ends = lambda c: [(p.w_end, p.adapt_after) for p in by[c]]
    # every = 7, K = 10: cuts at 7, 10, 14, 20, 21, ...; the update behind the multiples of 7 up to 70 only
    e = ends(Case(10, 1, 100, 0, 0, 0, 7, 70))
    assert e[:6] == [(7, 1), (10, 0), (14, 1), (20, 0), (21, 1), (28, 1)] and e[-3:] == [(80, 0), (90, 0), (100, 0)]
    assert sum(a for _, a in e) == 10
    # every a multiple of K: no launch more than without adaptation
    assert ends(Case(10, 1, 100, 0, 0, 0, 20, 80)) == [(10 * j, int(j % 2 == 0 and j <= 8)) for j in range(1, 11)]
    # every = 1: a launch a generation while it lasts
    assert ends(Case(10, 1, 40, 0, 0, 0, 1, 25)) == [(g, 1) for g in range(1, 26)] + [(30, 0), (40, 0)]
    # a snooker generation on an update position is followed by the update
    sn = [p for p in by[Case(10, 1, 60, 0, 0, 4, 12, 48)] if p.snooker and p.adapt_after]
    assert [p.g for p in sn] == [12, 24, 36, 48]
    # one past an update; ending on until
    assert ends(Case(10, 15, 30, 0, 0, 0, 14, 42))[:3] == [(20, 0), (28, 1), (30, 0)]
    assert ends(Case(10, 8, 35, 0, 0, 0, 7, 42))[-1] == (42, 1)
    # rng_offset 13: the positions 14, 21, ... are generations 1, 8, 15, ...
    assert [p.w_end for p in by[Case(10, 1, 50, 0, 13, 0, 7, 42)] if p.adapt_after] == [1, 8, 15, 22, 29]
    # lag 2: a launch over two K-windows is cut at 7 and 14
    assert ends(Case(10, 1, 90, 2, 0, 0, 7, 70))[:4] == [(7, 1), (14, 1), (20, 0), (21, 1)]
    # off: the plain schedule
    assert ends(Case(10, 1, 30, 0, 0, 0, 0, 0)) == [(10, 0), (20, 0), (30, 0)]


def test_what_the_executor_relies_on(walked):
    for c, launches in zip(CASES, walked):
        g_to = c.g_from + c.length - 1
        assert launches[0].g == c.g_from and launches[-1].w_end == g_to, c
        assert all(a.w_end + 1 == b.g for a, b in zip(launches, launches[1:])), c
        updates = {g for g in range(c.g_from, g_to + 1) if c.every and (g + c.rng_offset) % c.every == 0 and g + c.rng_offset <= c.until}
        assert {p.w_end for p in launches if p.adapt_after} == updates, c
        for p in launches:
            assert p.g <= p.w_end
            assert not any(p.g <= u < p.w_end for u in updates), (c, p)
            inside = [c.every > 0 and g + c.rng_offset <= c.until for g in range(p.g, p.w_end + 1)]
            assert all(v == bool(p.accumulate) for v in inside), (c, p)
            assert p.snooker == int(bool(c.snooker) and (p.g + c.rng_offset) % c.snooker == 0) and (not p.snooker or p.g == p.w_end), (c, p)
