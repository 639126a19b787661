"""CPU tier of the grouped demcz_run_checked: the launch-span sizing and the slab grouping of demc.jl_amd/csrc/demcz_slab_plan.h
(host code, no device), built into a stand-alone program under AddressSanitizer and UBSan and run as a program."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REC_PAD = 64


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("slab_plan") / "slab_plan_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "c_abi" / "slab_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr

    def run(*args):
        p = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr)
        return [[int(x) for x in line.split()] for line in p.stdout.splitlines()]

    return run


@pytest.fixture(scope="module")
def consts(plan):
    limit, tail, most, mib = plan("consts")[0]
    return {"limit": limit, "tail": tail, "most": most, "mib": mib}


def slab_of(g, every):
    return (g - 1) // every


# (g_from, g_to, every, span, cut, max_slabs); span 0: no bound
CASES = [
    (1, 10000, 1000, 5850, 0, 64),          # the benchmark's call
    (2001, 22000, 1000, 5850, 0, 64),       # a second call of 20 slabs
    (1, 10000, 1000, 1170, 0, 64),          # a span of one slab and a bit
    (1, 10000, 1000, 700, 0, 64),           # a span shorter than a slab
    (1, 1200, 100, 0, 0, 64),               # no bound on the span (a redo, one launch per K-window)
    (1, 1200, 4, 5850, 0, 64),              # 300 slabs: the bound on the slabs of a group
    (1, 1200, 4, 5850, 0, 7),               # ... and a smaller one from the caller
    (351, 6000, 1000, 5850, 0, 64),         # starts mid-slab
    (1, 5500, 1000, 5850, 0, 64),           # `every` does not divide the range: the last slab is partial
    (351, 5432, 1000, 2500, 0, 64),         # both
    (1, 1200, 200, 5850, 401, 64),          # armed at a slab start
    (1, 1200, 200, 5850, 450, 64),          # ... mid-slab
    (1, 1200, 200, 5850, 5000, 64),         # ... beyond the call
    (1, 1200, 4, 5850, 1120, 64),           # ... at a slab end
    (1, 700, 1000, 5850, 0, 64),            # less than one slab
    (1, 1000, 1000, 5850, 0, 64),           # exactly one
    (1, 2000, 1000, 5850, 0, 64),           # two
    (7, 7, 4, 1, 0, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_groups(plan, consts, case):
    g_from, g_to, every, span, cut, max_slabs = case
    groups = plan("groups", *case)
    # cover g_from..g_to exactly once, in order
    assert groups[0][0] == g_from and groups[-1][1] == g_to
    for (g0, e0, _), (g1, _, _) in zip(groups, groups[1:]):
        assert g1 == e0 + 1
    last_slab = slab_of(g_to, every)
    for i, (g, e, ends) in enumerate(groups):
        assert g <= e
        # ends on a slab end, or at g_to
        assert e % every == 0 or e == g_to
        assert ends == e // every - (g - 1) // every
        # the slab that holds g_to stands alone
        if slab_of(e, every) == last_slab:
            assert slab_of(g, every) == last_slab or g == g_from and slab_of(g_from, every) == last_slab
            assert i == len(groups) - 1
        slabs = slab_of(e, every) - slab_of(g, every) + 1
        # the span: a group of more than one slab never exceeds it
        if span > 0 and slabs > 1:
            assert e - g + 1 <= span
        assert slabs <= min(max_slabs, consts["most"])
        # the group in front of the last slab is short
        if i == len(groups) - 2:
            assert slabs <= consts["tail"]
        # a launch starts at the first slab end e with e + 1 >= cut
        if cut > g:
            assert e <= -(-(cut - 1) // every) * every
    if g_from < cut <= g_to:
        first = -(-(cut - 1) // every) * every
        if first < g_to:
            assert any(g == first + 1 for g, _, _ in groups), "no launch starts behind the armed generation's slab end"
    # as few groups as the rules allow where only the span binds: the benchmark's call
    if case == CASES[0]:
        assert [(g, e) for g, e, _ in groups] == [(1, 5000), (5001, 8000), (8001, 9000), (9001, 10000)]


def test_grouping_joins_slabs(plan):
    """(the point of it) ten slabs within the span are three calls, not ten: eight slabs, the one in front of the last, the last"""
    assert [r[:2] for r in plan("groups", 1, 10000, 1000, 10000, 0, 64)] == [[1, 8000], [8001, 9000], [9001, 10000]]
    assert [r[:2] for r in plan("groups", 1, 3000, 1000, 10000, 0, 64)] == [[1, 1000], [1001, 2000], [2001, 3000]]


GB = 10 ** 9


@pytest.mark.parametrize("archive", [0, 1 * GB, 32 * GB // 10, 37 * GB // 10], ids=["0", "1GB", "3.2GB", "3.7GB"])
@pytest.mark.parametrize("N,d,K,Gcap", [(1024, 5, 10, 12000), (64, 5, 10, 100), (2048, 5, 10, 0), (100000, 2, 10, 0), (1024, 5, 1000, 0)])
def test_span_sizing(plan, consts, archive, N, d, K, Gcap):
    for target_mib in (consts["mib"], 2 * consts["mib"], 64, 1024):
        gens, span, zb, rb, tb = plan("arena", archive, N, d, K, Gcap, target_mib << 20, REC_PAD)[0]
        per_gen = (d + 2) * N * 8
        if gens == 0:
            # no arena: not even 4 K generations fit beside this archive
            need = zb_of(archive) + 2 * (((4 * K * (d + 2) * N + REC_PAD) * 8 + 255) // 256 * 256) + ((4 * K + 64) * 8 + 255) // 256 * 256
            assert need >= consts["limit"]
            continue
        assert zb + 2 * rb + tb < consts["limit"]
        assert gens >= 4 * K
        assert zb == zb_of(archive) and rb >= (gens * (d + 2) * N + REC_PAD) * 8 and tb >= (gens + 64) * 8
        assert rb % 256 == 0 and tb % 256 == 0
        # the span is the target, or what fits; the buffers hold it, or the history window
        want = max(K, min((target_mib << 20) // per_gen, 1 << 20))
        assert K <= span <= want
        if span < want:      # shrunk: one generation more would not fit
            g1 = span + 1
            assert zb + 2 * (((g1 * (d + 2) * N + REC_PAD) * 8 + 255) // 256 * 256) + ((g1 + 64) * 8 + 255) // 256 * 256 >= consts["limit"]
        assert gens >= min(span, max(Gcap, 1024)) if Gcap > 0 else gens >= span


def zb_of(b):
    return (b + 255) // 256 * 256


def test_an_archive_of_3_7_gb_keeps_its_arena(plan, consts):
    gens, span, zb, rb, tb = plan("arena", 37 * GB // 10, 64, 5, 10, 100, consts["mib"] << 20, REC_PAD)[0]
    assert gens >= 1024 and span >= 40 and zb + 2 * rb + tb < consts["limit"]
