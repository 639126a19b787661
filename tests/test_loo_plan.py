"""CPU tier of the host half of PSIS-LOO: demcz_loo_host.h (host code, no device) -- the chunk planner of demcz_loo, the tail
length and the serial generalised-Pareto fit -- walked by a stand-alone program built under AddressSanitizer and UBSan
(tests/c_abi/loo_host_main.cpp), and held to tests/loo_reference.py and to the library's own exports of the same text."""
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import loo_reference as lr

ROOT = Path(__file__).resolve().parent.parent
GIB = 1 << 30


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("loo_host")
    exe = tmp / "loo_host_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", str(ROOT / "tests" / "c_abi" / "loo_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr

    def run(mode, payload):
        path = tmp / f"{mode}.in"
        if isinstance(payload, bytes):
            path.write_bytes(payload)
        else:
            path.write_text(payload)
        p = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:], p.stdout[-500:])
        return p.stdout.splitlines()

    return run


def plan_cases():
    cases = []
    for nobs in (1, 2, 31, 32, 33, 64, 70, 1000):
        for S in (1, 480, 10 ** 6, 2 ** 31 - 1):
            for budget in (0, 1, 24 * S - 1, 24 * S, 24 * S * 7 + 5, 24 * S * 32, 4 * GIB, 2 ** 62):
                cases.append((nobs, S, budget))
    return cases


def test_chunks_tile_the_observations_within_the_budget(host):
    cases = plan_cases()
    lines = iter(host("plan", "".join(f"{n} {S} {b}\n" for n, S, b in cases)))
    widths = set()
    for nobs, S, budget in cases:
        _, mc, nchunks = next(lines).split()
        mc, nchunks = int(mc), int(nchunks)
        widths.add(mc)
        assert 1 <= mc <= 32
        assert mc == max(1, min(32, budget // (24 * S))), (nobs, S, budget)      # the largest width that fits, and at least 1
        assert nchunks == -(-nobs // mc)
        at = 0
        for _ in range(nchunks):
            f, c = (int(v) for v in next(lines).split())
            assert f == at and 1 <= c <= mc and (c == mc or f + c == nobs)
            at += c
        assert at == nobs
        assert next(lines).split() == [str(nobs), "0"]                            # past the end: nothing
    assert widths >= {1, 7, 32}


def test_the_budget_of_the_library_is_four_gib():
    text = (ROOT / "demc.jl_amd" / "csrc" / "demcz_loo_host.h").read_text()
    assert re.search(r"LOO_SCRATCH_BUDGET = \(int64_t\)4 << 30;", text) and re.search(r"LOO_BYTES_PER_DRAW_COLUMN = 24;", text)
    assert re.search(r"LOO_MAX_CHUNK = 32;", text)


def test_tail_length_is_the_references(host, demc):
    cases = [(S, r) for S in (1, 2, 5, 400, 8000, 168000, 10 ** 6, 2 ** 31 - 1) for r in (1.0, 0.25, 0.3, 1.7, 4.0, 1e-9, 1e9)]
    out = host("tail", "".join(f"{S} {r!r}\n" for S, r in cases))
    for (S, r), line in zip(cases, out):
        rc, M = (int(v) for v in line.split())
        assert rc == 0 and M == lr.tail_cap(S, r) == demc.psis_tail_length(S, r) and 0 <= M <= max(0, S - 1)
    out = host("tail", "0 1.0\n10 0.0\n10 -1.0\n10 inf\n10 nan\n")
    assert [int(l.split()[0]) for l in out] == [1] * 5


@pytest.mark.parametrize("n,k", [(5, 0.2), (257, -0.3), (1230, 0.7)])
def test_serial_fit_under_the_sanitizers_is_the_librarys_and_the_references(host, demc, n, k):
    p = (np.arange(1, n + 1) - 0.5) / n
    x = 1.5 * ((1.0 - p) ** (-k) - 1.0) / k
    out = host("fit", struct.pack("q", n) + x.tobytes())
    rc, *hexes = out[0].split()
    got = [struct.unpack("d", struct.pack("Q", int(h, 16)))[0] for h in hexes]
    assert int(rc) == 0 and len(out) == 4
    lib = demc.gpd_fit(x)
    W = lr._Wide()
    kw, sw = lr.gpd_fit_ext(W.lift(x), W)
    for g, l, r, scale in zip(got, lib, (float(kw), float(sw), (n * float(kw) + 5) / (n + 10)), (1.0, 1.5, 1.0)):
        assert abs(g - r) <= scale * lr.KHAT_TOL and abs(l - r) <= scale * lr.KHAT_TOL
    smoothed = [struct.unpack("d", struct.pack("Q", int(h, 16)))[0] for h in out[1:]]
    assert smoothed[0] < smoothed[1] <= smoothed[2] <= 0.0


def test_fit_refuses_fewer_than_five(host):
    out = host("fit", struct.pack("q", 4) + np.arange(1.0, 5.0).tobytes())
    assert out[0].split()[0] == "1" and len(out) == 1
