"""CPU tier of the rank tests: the library's demcz_rank_to_z (host code, no device) against the NumPy restatement of
rank_reference.py bit for bit; the restatement against the true normal quantile in mpmath; the symmetries of the score; the declared
surface; the statistic composed from the existing extended-precision references on the two worlds it exists for; the conditions
that give the worlds of test_gpu_rank.py their meaning; and the shared header built into a stand-alone program under
AddressSanitizer and UBSan."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import quantile_cases as Q
import rank_cases as K
import rank_reference as RR
import stats_cases as S
import stats_reference as SR

ROOT = Path(__file__).resolve().parent.parent
GRID_S = (1, 2, 3, 7, 64, 1000)
BIG_S = 2 ** 40
# The largest error of the restated PPND16 against the true normal quantile at the double u, measured on the grids below: 4.72 ulp
# (at S = 2^40, u = 0.17705...; 4.08 on the small grids, 3.76 on the log-spaced u).  The grid is a sample: the bound is twice the
# measured maximum, rounded up to a whole ulp.
MEASURED_ULP = 4.72
BOUND_ULP = math.ceil(2 * MEASURED_ULP)


def half_ranks(S_):
    return np.arange(2, 2 * S_ + 1) / 2.0


def random_ranks():
    return np.random.default_rng(1).integers(2, 2 * BIG_S + 1, size=10000) / 2.0


# ---- (a) the library against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", GRID_S)
def test_rank_to_z_equals_the_restatement_on_every_half_rank(demc, S_):
    r = half_ranks(S_)
    assert np.array_equal(RR.bits(demc.rank_to_z(r, S_)), RR.bits(RR.rank_to_z(r, S_)))


def test_rank_to_z_equals_the_restatement_at_two_to_the_forty(demc):
    r = random_ranks()
    assert np.array_equal(RR.bits(demc.rank_to_z(r, BIG_S)), RR.bits(RR.rank_to_z(r, BIG_S)))
    ends = np.array([1.0, 1.5, 2.0, BIG_S - 0.5, float(BIG_S)])
    assert np.array_equal(RR.bits(demc.rank_to_z(ends, BIG_S)), RR.bits(RR.rank_to_z(ends, BIG_S)))


def test_rank_to_z_rejects_invalid_arguments(demc):
    for r, S_ in [([0.5], 10), ([10.5], 10), ([np.nan], 10), ([1.0], 0), ([1.0], 2 ** 50)]:
        with pytest.raises(demc.DemczError) as ei:
            demc.rank_to_z(r, S_)
        assert ei.value.code == 1, (r, S_)
    assert demc.rank_to_z([], 5).size == 0


# ---- (b) the restatement against the true normal quantile ----------------------------------------------------------------------------
def test_restatement_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    root2 = mp.sqrt(2)

    def worst(u, upper=False):
        """max error in ulp of the score at the double u: -ppnd16(u) against the quantile of the exact 1 - u for the upper side"""
        z = RR.ppnd16_lower(u)
        out = 0.0
        for a, b in zip(z.tolist(), u.tolist()):
            t = root2 * mp.erfinv(1 - 2 * mp.mpf(b)) if upper else root2 * mp.erfinv(2 * mp.mpf(b) - 1)
            a = -a if upper else a
            if t == 0:
                assert a == 0.0
                continue
            out = max(out, float(abs(mp.mpf(a) - t) / mp.mpf(float(np.spacing(abs(float(t)))))))
        return out

    figures = {}
    for S_ in GRID_S:
        upper, u = RR.blom_u(half_ranks(S_), S_)
        figures[f"S={S_}"] = worst(u[~upper])
    figures["S=2^40"] = worst(RR.blom_u(random_ranks(), BIG_S)[1])
    logu = np.logspace(-15, np.log10(0.5), 2000)
    figures["log-spaced, lower"] = worst(logu)
    figures["log-spaced, upper"] = worst(logu, upper=True)
    print("[rank] PPND16 restatement against mpmath, largest error in ulp:", {k: round(v, 2) for k, v in figures.items()})
    assert max(figures.values()) <= BOUND_ULP, figures


# ---- (c) symmetries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", GRID_S + (BIG_S,))
def test_score_is_odd_increasing_and_zero_at_the_centre(demc, S_):
    r = half_ranks(S_) if S_ != BIG_S else np.sort(np.concatenate([random_ranks(), [(BIG_S + 1) / 2.0]]))
    z = demc.rank_to_z(r, S_)
    zm = demc.rank_to_z((S_ + 1.0) - r, S_)
    assert np.array_equal(RR.bits(z + 0.0), RR.bits(-zm + 0.0))                     # odd about (S + 1) / 2, to the bit
    assert (np.diff(z[np.concatenate([[True], np.diff(r) > 0])]) > 0).all()       # strictly increasing in r
    centre = demc.rank_to_z([(S_ + 1) / 2.0], S_)
    assert centre[0] == 0.0 and np.isfinite(z).all()


# ---- (d) the surface -----------------------------------------------------------------------------------------------------------------
NEW = ["demcz_rank_to_z", "demcz_rank_normalize", "demcz_rank_normalize_array", "demcz_indicator_le", "demcz_rank_diagnostics",
       "demcz_rank_diagnostics_array"]


def test_new_symbols_are_declared_bound_and_exported(demc):
    import ctypes
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "demcz.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(demc.LIB_PATH))
    jl = (ROOT / "julia" / "DEMCHip.jl").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in demc.SYMBOLS and hasattr(lib, name), name
        assert f"(:{name}, libdemcz)" in jl, name
    assert re.search(r"#define DEMCZ_RANK_Z 0\b", hdr) and re.search(r"#define DEMCZ_RANK_AVERAGE 1\b", hdr)
    assert "without rank normalisation" not in (ROOT / "include" / "demcz.h").read_text()
    for name in ("rank_normalize_chain", "rank_diagnostics_chain", "rank_to_z", "RankDiagnostics"):
        assert hasattr(demc, name), name
    for name in ("rank_normalize", "indicator_le", "rank_diagnostics"):
        assert hasattr(demc.HipEngine, name) and hasattr(demc.DerivedHistory, name), name


# ---- (e) the statistic from the existing references ----------------------------------------------------------------------------------
def test_independent_normal_chains_look_converged():
    chain = K.independent_normal()
    N, d, G = chain.shape
    rhat, bulk, tail, _ = RR.diagnostics(chain)
    print(f"[rank] independent normal chains: rhat_rank {rhat}, ess_bulk {bulk}, ess_tail {tail}, S = {N * G}")
    assert (rhat < 1.01).all()
    for e in (bulk, tail):
        assert (e > N * G / 2).all() and (e < 2 * N * G).all()


def test_a_scale_mixture_is_seen_by_the_rank_statistic_only():
    chain = K.scale_mixture()
    plain = SR.rhat_gelman(chain)
    rhat, _, _, parts = RR.diagnostics(chain)
    print(f"[rank] scale mixture: plain R-hat {plain}, rhat_rank {rhat} (bulk {parts['rhat_bulk']}, folded {parts['rhat_folded']})")
    assert (plain < 1.01).all() and (rhat > 1.1).all()
    assert (parts["rhat_folded"] > parts["rhat_bulk"]).all()                       # the folded half is the one that sees it


# ---- (f) the worlds of test_gpu_rank.py reach what they are for ----------------------------------------------------------------------
def test_the_array_worlds_reach_their_shapes():
    a, b, c = K.ARRAY_WORLDS
    assert a[0] * a[2] < 64 and a[0] % 2 and a[1] % 2 and a[2] % 2
    assert b[0] % 64 and K.tile_count(b) > 8 and (b[0] * b[2]) % K.TILE
    assert K.tile_count(c) > 256


def test_the_tie_worlds_tie_where_they_should():
    x = K.all_equal()
    assert np.unique(x[:, 0]).size == 1 and np.unique(x[:, 1]).size == x.shape[0] * x.shape[2]
    r = RR.ranks_of_chain(x)
    assert (r[:, 0] == (x.shape[0] * x.shape[2] + 1) / 2).all() and (RR.z_of_ranks(r)[:, 0] == 0.0).all()
    for p in range(2):                                                  # low byte: seven constant digits, the lowest decides
        k = Q.keys(Q.draws(K.low_byte(), p))
        assert np.unique(k >> np.uint64(8)).size == 1 and np.unique(k & np.uint64(255)).size > 200
    k = Q.keys(Q.draws(K.sign_only(), 0))
    assert np.unique(k).size == 2 and all(np.unique((k >> np.uint64(8 * b)) & np.uint64(255)).size == 2 for b in range(8))
    k = Q.keys(Q.draws(K.high_byte_only(), 0))
    digits = [np.unique((k >> np.uint64(8 * b)) & np.uint64(255)).size for b in range(8)]
    assert digits == [1] * 7 + [5], digits                              # seven of eight digits constant: the skip path
    s = Q.draws(K.specials(), 0)
    assert (np.signbit(s) & (s == 0)).sum() >= 10 and (~np.signbit(s) & (s == 0)).sum() >= 10 and np.isinf(s).sum() == 6
    assert (np.abs(s[s != 0]) < 2.3e-308).sum() == 8
    r = RR.ranks_of_chain(K.specials())[:, 0]
    assert np.unique(r[K.specials()[:, 0] == 0]).size == 1              # -0.0 and +0.0 share one rank
    k = Q.keys(Q.draws(K.specials(), 1))
    assert all(np.unique((k >> np.uint64(8 * b)) & np.uint64(255)).size > 1 for b in range(8))      # every digit pass runs


def test_the_nan_world_and_the_lattice():
    bad, clean = K.with_nan(), K.without_nan()
    assert np.isnan(bad).sum() == 1 and np.isnan(bad[:, 1]).any() and not np.isnan(clean).any()
    r = RR.ranks_of_chain(bad)
    assert np.isnan(r[:, 1]).all() and np.array_equal(r[:, [0, 2]], RR.ranks_of_chain(clean)[:, [0, 2]])
    x = K.lattice()
    for p in range(2):
        assert (x[:, p] == K.LATTICE_CENTER[p]).sum() >= 10             # fabs(0) ties
    folded = RR.ranks_of_chain(x, center=K.LATTICE_CENTER)
    assert np.unique(folded[:, 0]).size <= 9 and (folded != RR.ranks_of_chain(x)).any()


def test_the_run_world_rejects_most_proposals(demc, oracle):
    from helpers import oracle_sample
    a = K.RUN
    w = demc.workloads.iso_quad_problem(a["d"], a["N"])
    out = oracle_sample(oracle, w["target"], w["Zinit"], a["N"], a["K"], a["G"], [range(a["d"])], w["eps_scale"], a["gamma"], a["seed"])
    accept = SR.accept_ratio(out["log_obj"])
    held = (out["chain"][:, :, 1:] == out["chain"][:, :, :-1]).mean()
    print(f"[rank] run world: acceptance {accept.mean():.3f}, share of repeated values {held:.3f}")
    assert accept.mean() < 0.30 and held > 0.70
    r = RR.ranks_of_chain(out["chain"])
    assert (r != np.floor(r)).any() and (np.unique(r[:, 0]).size < r[:, 0].size / 2)      # runs of ties: far fewer ranks than draws


# ---- the shared header as a stand-alone program under the sanitizers ------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("rank_host") / "rank_host_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", str(ROOT / "tests" / "c_abi" / "rank_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    return exe


def _run_program(exe, tmp_path, S_, r):
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([S_, r.size], dtype=np.int64).tobytes() + np.ascontiguousarray(r, dtype=np.float64).tobytes())
    return subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("S_", GRID_S + (BIG_S,))
def test_the_score_under_the_sanitizers(sanitized_program, tmp_path, S_):
    r = half_ranks(S_) if S_ != BIG_S else random_ranks()
    out = _run_program(sanitized_program, tmp_path, S_, r)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    got = np.array([int(v, 16) for v in out.stdout.split()], dtype=np.uint64).reshape(2, r.size)
    want = RR.bits(RR.rank_to_z(r, S_))
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)


def test_the_program_reports_a_rejected_rank(sanitized_program, tmp_path):
    out = _run_program(sanitized_program, tmp_path, 4, np.array([1.0, 4.5]))
    assert out.returncode == 4 and "demcz_rank_to_z" in out.stderr
