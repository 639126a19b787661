"""CPU tier of the launch schedule with snooker generations: plan_launch of demc.jl_amd/csrc/demcz_run_plan.h (host code, no
device) walked over whole demcz_run calls by a stand-alone program built under AddressSanitizer and UBSan
(tests/c_abi/snooker_plan_main.cpp).  Whatever K, the call, the append lag and the position of the random streams:

  * the launches tile g_from..g_to exactly;
  * a launch is a snooker launch iff it is one generation long AT a snooker generation -- (g + rng_offset) % every == 0;
  * no other launch contains a snooker generation;
  * every K boundary of the call is counted by exactly one launch, and to_boundary is the distance to the next one;
  * between snooker generations the schedule is the one without them: a launch ends at a K boundary (lag 0), a batch end (lag E),
    the generation in front of a snooker generation, or the call's end -- nowhere else;
  * with every = 0 the plan is the one of a handle that has never heard of snooker generations."""
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("snooker_plan")
    exe = tmp / "snooker_plan_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "c_abi" / "snooker_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr

    def run(cases):
        (tmp / "cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
        p = subprocess.run([str(exe), "walk", str(tmp / "cases.txt")], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:], p.stdout[-500:])
        out, cur = [], None
        for line in p.stdout.splitlines():
            if line.startswith("case"):
                cur = []
                out.append(cur)
            else:
                cur.append(tuple(int(v) for v in line.split()))
        assert len(out) == len(cases)
        return out

    return run


def grid():
    """(K, g_from, length, every, rng_offset, E, external); caller-owned appends only on calls demcz_run admits with them"""
    cases = []
    for K in (1, 3, 10):
        for every in sorted({0, 1, 3, K, K + 1}):
            for g_from, length in itertools.product(sorted({1, 2, K, K + 1, 2 * K + 2}), sorted({1, 2, K, 4 * K + 3, 97})):
                g_to = g_from + length - 1
                for rng_offset, E, external in itertools.product((0, 5, 37), (0, 1, 2), (0, 1)):
                    nb = g_to // K - (g_from - 1) // K
                    if external and (E > 0 or nb > 1 or (nb == 1 and g_to % K != 0)):
                        continue
                    cases.append((K, g_from, length, every, rng_offset, E, external))
    return cases


def test_snooker_generations_are_launches_of_their_own(walk):
    cases = grid()
    assert any(c[3] == c[0] + 1 and c[4] > 0 for c in cases) and len(cases) > 2000
    seen_snooker_at_boundary = seen_cut_in_window = 0
    for c, launches in zip(cases, walk(cases)):
        K, g_from, length, every, off, E, external = c
        g_to = g_from + length - 1
        is_sn = lambda g: every > 0 and (g + off) % every == 0
        assert launches[0][0] == g_from and launches[-1][1] == g_to, c
        assert all(b[0] == a[1] + 1 for a, b in zip(launches, launches[1:])), c
        for g, w_end, to_boundary, nbound, snooker in launches:
            assert g <= w_end, c
            assert bool(snooker) == (w_end == g and is_sn(g)) == is_sn(g), (c, g)
            if not snooker:
                assert not any(is_sn(x) for x in range(g, w_end + 1)), (c, g, w_end)
            assert nbound == sum(1 for x in range(g, w_end + 1) if x % K == 0), (c, g)
            assert (g + to_boundary - 1) % K == 0 and 1 <= to_boundary <= K, (c, g)
            # where a launch may end
            batch_end = E > 0 and not external and w_end % (K * E) == 0
            assert w_end == g_to or is_sn(w_end + 1) or snooker or (w_end % K == 0 and (E == 0 or external)) or batch_end, (c, g, w_end)
            if E == 0:
                assert nbound <= 1 and (nbound == 0 or w_end % K == 0), (c, g, w_end)      # the rows of a boundary are visible to the next launch
            seen_snooker_at_boundary += bool(snooker and nbound)
            seen_cut_in_window += bool(not snooker and w_end != g_to and w_end % K != 0)
        assert sum(l[3] for l in launches) == g_to // K - (g_from - 1) // K, c
        assert sum(l[4] for l in launches) == sum(1 for g in range(g_from, g_to + 1) if is_sn(g)), c
    assert seen_snooker_at_boundary > 100 and seen_cut_in_window > 100


def test_every_zero_is_the_schedule_without_snooker(walk):
    """... which for a one-lane handle is: up to the next K boundary (lag 0) or batch end, or the call's end."""
    cases = [c for c in grid() if c[3] == 0]
    for c, launches in zip(cases, walk(cases)):
        K, g_from, length, _, _, E, external = c
        g_to, g, want = g_from + length - 1, g_from, []
        while g <= g_to:
            nb = -(-g // K) * K
            end = nb if (E == 0 or external) else -(-(nb // K) // E) * E * K
            end = min(end, g_to)
            want.append((g, end))
            g = end + 1
        assert [(l[0], l[1]) for l in launches] == want and not any(l[4] for l in launches), c


def test_two_calls_worked_by_hand(walk):
    """K = 3, generations 1..5, every third generation: 1-2, the snooker generation 3 (which is the boundary), 4-5.  The same call
    with the streams 1 generation on: generations 2 and 5 are the snooker generations."""
    assert walk([(3, 1, 5, 3, 0, 0, 0), (3, 1, 5, 3, 1, 0, 0)]) == [
        [(1, 2, 3, 0, 0), (3, 3, 1, 1, 1), (4, 5, 3, 0, 0)],
        [(1, 1, 3, 0, 0), (2, 2, 2, 0, 1), (3, 3, 1, 1, 0), (4, 4, 3, 0, 0), (5, 5, 2, 0, 1)]]
