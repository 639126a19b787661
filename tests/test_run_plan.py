"""CPU tier of demcz_run's launch schedule: demc.jl_amd/csrc/demcz_run_plan.h (host code, no device), built into a stand-alone
program under AddressSanitizer and UBSan and run as a program (tests/c_abi/run_plan_main.cpp).  The program walks whole calls as
demcz_run does -- plan a launch, admit the pending rows, hand the record descriptors over as pc_prepare does, book the appends --
and prints every launch's plan.

(a) `parent_walk` below is a second reading of the same schedule: the loop of demcz_run as it stood before the schedule moved
    into the header, restated in Python from that text (the way tests/golden/numpy_restatement.py restates the sampler).  The
    program's output equals it line for line over the grid.
(b) `check_properties` asserts what a schedule has to satisfy whatever the restatement says.

Two properties one might expect do NOT hold for the schedule as it has always been, and are asserted in the form that does:
  * with an append lag a launch ends at a batch end or at the call's end -- except a two-chain handle's regular launch, which is
    cut to whole passes and leaves fewer than one pass to a second launch;
  * a two-chain handle's irregular launch never crosses a K boundary -- with lag 0.  With a lag the launch covers its batch like
    any other: nothing appended inside a batch is visible inside it."""
import itertools
import re
import shutil
import subprocess
from collections import namedtuple
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

Case = namedtuple("Case", "K g_from length E span external shards peer split two_chain reg_facts desc rng_offset hint pending cold force_live")
Launch = namedtuple("Launch", "g w_end to_boundary nbound live dual next_g_first next_ngen next_M next_rows next_boff serves cur_ngen")


def boundary_at_or_after(g, K):
    return -(-g // K) * K


def boundaries_in(g, e, K):
    return e // K - (g - 1) // K


def grid():
    """The cross product of the parameters, without the combinations that cannot occur: demcz_run refuses caller-owned appends on
    a call that crosses more than its last generation's boundary, and they exclude a lag; live_span() is positive only on a split
    layout with lag 0, library-owned appends and -- with several shards -- the rows handed over inside the launches (`peer`, which
    in turn needs a span); a two-chain handle is a split layout; the record descriptors, the next-call hint and the cold-start
    limit bear on launches with a span only; rows are pending only under a lag, from boundaries before the call.
    The 1000-generation calls (up to 1000 launches each) vary the four parameters that bear on a call's first launch, its last
    one or the position of the random streams alone -- descriptor, cold-start limit, hint, offset -- together, not crossed: what
    they do to a call is the same whatever its length, and the shorter calls have the cross product."""
    cases = []
    for K in (1, 5, 7, 10):
        for g_from in sorted({1, 3, K, K + 1, 2 * K + 2}):
            for length in sorted({1, K - 1, K, 4 * K, 4 * K + 3, 1000} - {0}):
                g_to = g_from + length - 1
                ext_ok = boundaries_in(g_from, g_to, K) == 1 and g_to % K == 0
                for E, span, external in itertools.product((0, 1, 2, 3), (0, K, 25, 1170), (0, 1)):
                    if external and (E > 0 or not ext_ok or span > 0) or span > 0 and E > 0 or 0 < span < K:
                        continue
                    for shards, peer, split in ((1, 0, 0), (2, 0, 0), (1, 0, 1), (2, 0, 1), (2, 1, 1)):
                        if span > 0 and (not split or shards == 2 and not peer) or peer and span == 0:
                            continue
                        for two_chain, reg_facts in ((0, 0), (1, 1), (1, 0)):
                            if two_chain and not split:
                                continue
                            cold_far = 11983 // K * K          # (64 MiB of records at N = 100, d = 5)
                            for desc, hint, cold, rng_offset, pending in itertools.product((0, 1, 2, 3), (0, 40), (3 * K, cold_far), (0, 37), (0, 1)):
                                if span == 0 and (desc, hint, cold) != (0, 0, 3 * K):
                                    continue
                                if pending and (E == 0 or g_from <= K) or rng_offset and not split:
                                    continue
                                together = ((0, 0, 3 * K, 0), (1, 40, cold_far, 37), (2, 0, cold_far, 37), (3, 40, 3 * K, 0))
                                if length == 1000 and (desc, hint, cold, rng_offset) not in together:
                                    continue
                                cases.append(Case(K, g_from, length, E, span, external, shards, peer, split, two_chain, reg_facts,
                                                  desc, rng_offset, hint, pending, cold, 0))
    # DEMCZ_FORCE_LIVE_KERNEL: the LIVE kind whatever lies inside the launch
    cases += [c._replace(force_live=1) for c in cases if c.span > 0 and c.shards == 1 and not c.two_chain and c.desc == 1 and c.cold == 3 * c.K]
    return cases


def parent_walk(c, N, M0, R):
    """demcz_run's `while (g <= g_to)` loop with admit_pending, pc_prepare's descriptor hand-over and the append bookkeeping, in
    the order and the words of the C++ before the schedule was moved (h->X is X here; the handle starts as run_plan_main starts it)."""
    K, E, G = c.K, c.E, c.length
    g_to = c.g_from + c.length - 1
    rng_offset, plan_next = c.rng_offset, c.hint
    M = M_app = M0
    batch_J, pending = -1, []
    j0 = (c.g_from - 1) // K
    if c.pending and E > 0 and j0 >= 1:
        J1 = (j0 + E - 1) // E * E
        pending = [[J1 * K + 1, M0 + N * c.shards], [(J1 + E) * K + 1, M0 + 2 * N * c.shards]]
        M_app = M0 + 2 * N * c.shards
        batch_J = J1
    dc = dict(valid=False, g_first=0, M=0, rows=0, ngen=0, boff=0)
    if c.desc:
        dc = dict(valid=True, g_first=c.g_from + rng_offset, M=M + 7 if c.desc == 3 else M, rows=N * c.shards if E == 0 else 0,
                  ngen=K if c.desc == 2 else max(c.span, c.length), boff=K - (((c.g_from - 1) // K + 1) * K - c.g_from + 1))
    out = []
    g = c.g_from
    while g <= g_to:
        next_boundary = ((g - 1) // K + 1) * K
        w_end = min(next_boundary, g_to)
        if E > 0 and not c.external:
            jn = next_boundary // K
            J = ((jn + E - 1) // E) * E
            w_end = min(J * K, g_to)
        live_max = c.span
        dual_now = False
        if c.two_chain:
            tb0, rest = next_boundary - g + 1, g_to - g + 1
            reg = K % R == 0 and tb0 % R == 0 and rest >= R and bool(c.reg_facts)
            if reg:
                dual_now = True
                if live_max > 0:
                    live_max = max((min(live_max, rest) // R) * R, R)
                else:
                    w_end = g + ((w_end - g + 1) // R) * R - 1
            else:
                live_max = 0
        rows_v = N * (c.shards if c.peer else 1)
        boff = K - (next_boundary - g + 1)
        ready = dc["valid"] and dc["g_first"] == g + rng_offset and dc["M"] == M and dc["rows"] == rows_v and dc["boff"] == boff
        serves, cur_ngen = ready and dc["ngen"] >= K, dc["ngen"]
        if live_max > 0:
            n = min(live_max, g_to - g + 1)
            if ready and dc["ngen"] >= K:
                if dc["ngen"] < n:
                    n = max((dc["ngen"] // K) * K, K)
            else:
                n = min(n, c.cold)
            if dual_now:
                n = max((n // R) * R, R)
            w_end = g + n - 1
        while pending and pending[0][0] <= g:           # admit_pending
            M = pending.pop(0)[1]
        nbound = w_end // K - (g - 1) // K
        P = dict(M=M, g_first=g + rng_offset, ngen=w_end - g + 1, to_boundary=next_boundary - g + 1)
        nxt = (0, 0, 0, 0, 0)
        if c.split:
            ng = w_end + 1
            nb1 = ((ng - 1) // K + 1) * K
            nend = nb1
            if E > 0 and not c.external:
                nend = ((nend // K + E - 1) // E) * E * K
            nM, nn = M, nend - ng + 1
            rows_n = N * c.shards
            if live_max > 0:
                nn = min(live_max, g_to - w_end if w_end < g_to else (plan_next if plan_next > 0 else G))
            if c.external:
                nn = 0
            elif E == 0:
                nM = M_app + nbound * rows_n
            else:
                for vis, M_after in pending:
                    if vis <= ng:
                        nM = M_after
            vis_rows = rows_n if E == 0 else 0
            nboff = K - (nb1 - ng + 1)
            nxt = (ng + rng_offset, nn, nM, vis_rows, nboff)
            # pc_prepare(h, P, vis_rows, ng + rng_offset, nn, nM, vis_rows, nboff)
            cur_boff = K - P["to_boundary"]
            if not (dc["valid"] and dc["g_first"] == P["g_first"] and dc["ngen"] >= P["ngen"] and dc["M"] == P["M"]
                    and dc["rows"] == vis_rows and dc["boff"] == cur_boff):
                dc = dict(valid=True, g_first=P["g_first"], M=P["M"], ngen=P["ngen"], rows=vis_rows, boff=cur_boff)
            dc = dict(valid=nn > 0, g_first=ng + rng_offset, M=nM, ngen=max(nn, 0), rows=vis_rows, boff=nboff)       # rec_cur ^= 1
        live = live_max > 0 and (((w_end - 1) // K - (g - 1) // K) > 0 or bool(c.peer) or bool(c.force_live))
        out.append(Launch(g, w_end, next_boundary - g + 1, nbound, int(live), int(dual_now), *nxt, int(serves), cur_ngen))
        if w_end < g:
            break
        if nbound > 0 and not c.external:
            rows = N * c.shards
            if E == 0:
                M_app += nbound * rows
                M = M_app
            else:
                for j in range((g - 1) // K + 1, w_end // K + 1):
                    J = ((j + E - 1) // E) * E
                    M_app += rows
                    if batch_J != J:
                        pending.append([(J + E) * K + 1, M_app])
                        batch_J = J
                    else:
                        pending[-1][1] = M_app
        g = w_end + 1
    return out


def check_properties(c, launches, R):
    K, E, span = c.K, c.E, c.span
    g_to = c.g_from + c.length - 1
    # the launches cover g_from..g_to once, in order
    assert launches[0].g == c.g_from and launches[-1].w_end == g_to
    for a, b in zip(launches, launches[1:]):
        assert b.g == a.w_end + 1
    for p in launches:
        n, rest = p.w_end - p.g + 1, g_to - p.g + 1
        inside = boundaries_in(p.g, p.w_end - 1, K)          # boundaries strictly inside: later generations draw from their rows
        assert p.g <= p.w_end <= g_to
        assert p.nbound == boundaries_in(p.g, p.w_end, K)
        assert p.to_boundary == boundary_at_or_after(p.g, K) - p.g + 1
        if span == 0 and E == 0:
            assert p.nbound <= 1 and (p.nbound == 0 or p.w_end % K == 0)
        if E > 0 and not c.external:
            # (a two-chain handle's regular launch is cut to whole passes: fewer than R generations are left to the call's end)
            assert p.w_end == g_to or p.w_end % (E * K) == 0 or p.dual and g_to - p.w_end < R and g_to < boundary_at_or_after(p.g, E * K)
        if p.live:
            assert n <= span
            assert inside > 0 or c.peer or c.force_live
        if span == 0:
            assert not p.live
        if p.dual:
            assert c.two_chain and K % R == 0 and p.to_boundary % R == 0 and n % R == 0 and n >= R
        if c.two_chain and not p.dual and E == 0:
            assert inside == 0
        if c.split:
            assert p.next_g_first - c.rng_offset == p.w_end + 1
            assert p.next_boff == K - (boundary_at_or_after(p.w_end + 1, K) - p.w_end)
            if c.external:
                assert p.next_ngen == 0
        may_span = span > 0 and (not c.two_chain or p.dual)      # (an irregular launch of a two-chain handle has no span)
        if may_span and p.serves and p.cur_ngen < min(span, rest):
            assert n <= max(p.cur_ngen // K * K, K)
        if may_span and not p.serves:
            assert n <= max(c.cold, R if p.dual else 0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("run_plan")
    exe = tmp / "run_plan_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "c_abi" / "run_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr

    def run(*args):
        p = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:], p.stdout[-500:])
        return p.stdout

    return run, tmp


@pytest.fixture(scope="module")
def walked(program):
    """every case of the grid with the launches the program planned for it"""
    run, tmp = program
    N, M0, R = (int(x) for x in run("consts").split())
    cases = grid()
    (tmp / "cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    walks = []
    for line in run("walk", tmp / "cases.txt").splitlines():
        if line.startswith("case "):
            assert int(line.split()[1]) == len(walks)
            walks.append([])
        else:
            walks[-1].append(Launch(*(int(x) for x in line.split())))
    assert len(walks) == len(cases)
    return cases, walks, (N, M0, R)


def test_the_grid_reaches_every_kind_of_launch(walked):
    cases, walks, _ = walked
    assert len(cases) > 5000
    seen = {(p.live, p.dual, p.serves, p.nbound > 1) for w in walks for p in w}
    for live, dual, serves in itertools.product((0, 1), repeat=3):
        assert any(s[:3] == (live, dual, serves) for s in seen), (live, dual, serves)
    assert any(c.two_chain and c.span > 0 and not p.dual for c, w in zip(cases, walks) for p in w)
    assert any(c.span > 0 and not p.serves and p.w_end - p.g + 1 == c.cold < min(c.span, c.length) for c, w in zip(cases, walks) for p in w[:1])


def test_the_plan_equals_the_loop_it_replaced(walked):
    cases, walks, (N, M0, R) = walked
    for c, got in zip(cases, walks):
        want = parent_walk(c, N, M0, R)
        assert got == want, (c, [(a, b) for a, b in zip(got, want) if a != b][:1], len(got), len(want))


def test_the_schedule_has_its_properties(walked):
    cases, walks, (_, _, R) = walked
    for c, launches in zip(cases, walks):
        try:
            check_properties(c, launches, R)
        except AssertionError as e:
            raise AssertionError(f"{c}: {launches[:4]} ...") from e


def test_a_malformed_case_is_an_error(program):
    """(the program tells by its exit code: 2 a case it cannot read, 3 a launch that made no progress -- which no case of the grid does)"""
    _, tmp = program
    (tmp / "bad.txt").write_text("5 1 10 0\n")
    p = subprocess.run([str(tmp / "run_plan_main"), "walk", str(tmp / "bad.txt")], capture_output=True, text=True)
    assert p.returncode == 2
