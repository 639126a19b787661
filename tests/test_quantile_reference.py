"""CPU tier of the quantile tests: the key order and the reference of quantile_cases.py; the radix select digit by digit, with
np.bincount standing in for the counting kernel and the library's own demcz_select_step, demcz_quantile_plan and
demcz_quantile_finish (host code, no device) through ctypes; the preconditions that give the cases of test_gpu_quantiles.py their
meaning; the declared surface; and the same three finishers built into a stand-alone program under AddressSanitizer and UBSan."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import quantile_cases as Q
import stats_cases as S

ROOT = Path(__file__).resolve().parent.parent
FINITE_WORLDS = Q.ARRAY_WORLDS + ["low_byte", "repeated", "identical", "one_draw"]
ALL_WORLDS = FINITE_WORLDS + ["specials"]


def chain_of(w):
    if isinstance(w, tuple):
        return S.world(*w)
    return {"low_byte": Q.low_byte_world, "repeated": Q.repeated_world, "identical": S.all_identical, "one_draw": Q.one_draw,
            "specials": Q.specials}[w]()


def wid(w):
    return Q.ids(w) if isinstance(w, tuple) else w


def select_on_host(demc, chain, probs, shards=1):
    """The selection as sampler._Runner.quantiles drives it, the counting pass in NumPy: `shards` pieces of the chains counted
    separately and added."""
    N, d, G = chain.shape
    cut = [N * s // shards for s in range(shards + 1)]
    pieces = [chain[a:b] for a, b in zip(cut[:-1], cut[1:]) if b > a]

    def count_pass(shift, prefix):
        parts = [Q.count_pass(c, shift, prefix) for c in pieces]
        return sum(c for c, _ in parts), sum(n for _, n in parts)

    return demc.select_quantiles(count_pass, N * G, d, probs)


# ---- (a) the order -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", FINITE_WORLDS, ids=wid)
def test_key_order_is_numeric_order_on_finite_worlds(w):
    chain = chain_of(w)
    for p in range(chain.shape[1]):
        x = Q.draws(chain, p)
        assert np.array_equal(Q.from_keys(np.sort(Q.keys(x))), np.sort(x))
        assert np.array_equal(Q.from_keys(Q.keys(x)).view(np.uint64), x.view(np.uint64))


def test_key_order_of_the_special_values():
    neg_nan = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]
    want = np.array([neg_nan, -np.inf, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan])
    k = Q.keys(want)
    assert (np.diff(k.astype(object)) > 0).all()                       # strictly increasing as unsigned integers
    shuffled = want[np.random.default_rng(0).permutation(want.size)]
    assert np.array_equal(Q.from_keys(np.sort(Q.keys(shuffled))).view(np.uint64), want.view(np.uint64))
    assert int(k[0]) == 0x0007FFFFFFFFFFFF and int(k[3]) == 0x7FFFFFFFFFFFFFFF and int(k[4]) == 0x8000000000000000


# ---- (b) digit by digit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", ALL_WORLDS, ids=wid)
def test_selection_by_counts_lands_on_the_reference(demc, w):
    chain = chain_of(w)
    ref = Q.reference(chain)
    got = select_on_host(demc, chain, Q.PROBS)
    assert Q.same(got, ref)
    if chain.shape[0] >= 3:
        assert Q.same(select_on_host(demc, chain, Q.PROBS, shards=3), ref)


@pytest.mark.parametrize("negative", [False, True], ids=["+nan", "-nan"])
def test_a_nan_spoils_its_own_parameter_only(demc, negative):
    bad, clean = Q.with_nan(negative), Q.reference(Q.specials())
    ref = Q.reference(bad)
    got = select_on_host(demc, bad, Q.PROBS, shards=3)
    assert Q.same(got, ref)
    assert np.isnan(got.q[1]).all() and np.isnan(got.lower[1]).all() and np.isnan(got.upper[1]).all()
    for a, b in zip(got, clean):
        assert np.array_equal(Q.bits(a[[0, 2]]), Q.bits(b[[0, 2]]))


def test_select_step_walks_one_byte_and_rejects_a_rank_outside_the_counts(demc):
    counts = np.zeros((2, 2, 256), dtype=np.int64)
    counts[0, 0, [3, 7, 200]] = [2, 5, 1]
    counts[0, 1] = counts[0, 0]
    counts[1, :, 255] = 9
    prefix = np.array([[0x12, 0x12], [0, 0]], dtype=np.uint64)
    rank = np.array([[1, 7], [0, 8]], dtype=np.int64)
    p2, r2 = demc.select_step(counts, prefix, rank)
    assert p2.tolist() == [[0x1203, 0x12C8], [0xFF, 0xFF]] and r2.tolist() == [[1, 0], [0, 8]]
    assert prefix.tolist() == [[0x12, 0x12], [0, 0]]                  # (the caller's arrays are not written)
    for bad in ([[1, 8], [0, 8]], [[1, 7], [0, 9]], [[-1, 7], [0, 8]]):
        with pytest.raises(demc.DemczError) as ei:
            demc.select_step(counts, prefix, np.array(bad, dtype=np.int64))
        assert ei.value.code == 1


# ---- (c) plan and finish -------------------------------------------------------------------------------------------------------------
def test_plan_equals_the_restated_formula(demc):
    probs = list(Q.PROBS) + [0.1, 0.9999999999999999, 5e-324, 0.5, 0.5, 0.3]
    for S_ in (1, 2, 3, 10, 257 * 40, 24600, 2 ** 31 + 5, 2 ** 53 + 2, 2 ** 62):
        for chunk in (probs[:8], probs[8:], probs[::-1][:16]):
            lo, hi, frac = demc.quantile_plan(S_, chunk)
            rlo, rhi, rfrac = Q.plan(S_, chunk)
            assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi) and np.array_equal(Q.bits(frac), Q.bits(rfrac)), S_
            assert (0 <= lo).all() and (lo <= hi).all() and (hi <= S_ - 1).all()


def test_plan_and_finish_reject_invalid_arguments(demc):
    for S_, probs in [(0, [0.5]), (-3, [0.5]), (10, []), (10, [0.5] * 17), (10, [-0.1]), (10, [0.5, np.nan]), (10, [1.0000000000000002]),
                      (10, [np.inf])]:
        with pytest.raises(demc.DemczError) as ei:
            demc.quantile_plan(S_, probs)
        assert ei.value.code == 1, (S_, probs)
    assert demc.quantile_plan(10, [0.5] * 16)[0].tolist() == [4] * 16 and demc.quantile_plan(10, [1.0, 0.0])[0].tolist() == [9, 0]
    k = np.zeros((2, 17), dtype=np.uint64)
    with pytest.raises(demc.DemczError) as ei:
        demc.quantile_finish(k, k, np.zeros(17))
    assert ei.value.code == 1


def test_finish_equals_the_restated_formula(demc):
    a = np.array([1.0, -np.inf, -np.inf, 0.0, -0.0, 1e308, -1e308, 5e-324, 3.0, 1.0, np.inf])
    b = np.array([2.0, 1.0, np.inf, 0.0, 0.0, 1.7e308, 1e308, 1e-323, 3.0, np.inf, np.inf])
    frac = np.array([0.0, 0.5, 1.0 / 3.0, 0.999999, 5e-324])
    for f in frac:
        got = demc.quantile_finish(Q.keys(a)[None, :].repeat(2, axis=0), Q.keys(b)[None, :].repeat(2, axis=0), np.full(a.size, f)[:11],
                                   np.array([0, 4]))
        want = np.array([Q.combine(x, y, f) for x, y in zip(a, b)])
        assert np.array_equal(Q.bits(got.q[0]), Q.bits(want)), f
        assert np.array_equal(Q.bits(got.lower[0]), Q.bits(a)) and np.array_equal(Q.bits(got.upper[0]), Q.bits(b))
        for x in got:                                                  # the second parameter holds NaNs: NaN everywhere
            assert np.array_equal(Q.bits(x[1]), Q.bits(np.full(a.size, np.nan)))


@pytest.mark.parametrize("w", FINITE_WORLDS, ids=wid)
def test_agrees_with_numpy_quantile(demc, w):
    """np.quantile's type 7 forms a + (b - a) g by another sequence of roundings (and from the other end for g >= 0.5): the two
    differ by a few units of 2^-53 max(|a|, |b|); the bound is 4 of them."""
    chain = chain_of(w)
    got = select_on_host(demc, chain, Q.PROBS)
    worst = 0.0
    for p in range(chain.shape[1]):
        want = np.quantile(Q.draws(chain, p), Q.PROBS)
        scale = np.maximum(np.abs(got.lower[p]), np.abs(got.upper[p]))
        err = np.abs(got.q[p] - want)
        assert (err <= 4 * 2.0 ** -53 * scale).all(), (p, err, scale)
        worst = max(worst, float(np.max(err[scale > 0] / (2.0 ** -53 * scale[scale > 0]), initial=0.0)))
    print(f"[quantiles] {wid(w)}: worst difference to np.quantile {worst:.2f} units of 2^-53 max(|a|, |b|)")


# ---- (d) preconditions -----------------------------------------------------------------------------------------------------------------
def test_the_hot_parameter_fills_one_bin_in_the_first_three_passes():
    chain = S.world(*Q.HOT_WORLD)
    x = Q.draws(chain, Q.HOT_PARAMETER)
    assert abs(x.mean() - 1e6) < 1 and 0.5 < x.std() < 2
    share = Q.bin_share(chain, Q.HOT_PARAMETER)
    assert share[:3] == [1.0, 1.0, 1.0] and 0.05 < share[3] < 1.0, share
    zero_mean = Q.bin_share(chain, 0)
    assert zero_mean[0] < 0.6, zero_mean                              # (a parameter around zero spreads over both signs at once)


def test_the_low_byte_world_is_decided_by_the_last_pass_alone():
    chain = Q.low_byte_world()
    for p in range(2):
        b = Q.draws(chain, p).view(np.uint64)
        assert np.unique(b >> np.uint64(8)).size == 1 and np.unique(b & np.uint64(255)).size > 100
        assert Q.bin_share(chain, p)[:7] == [1.0] * 7
    assert (chain[:, 0] > 0).all() and (chain[:, 1] < 0).all()


def test_the_repeated_world_repeats_and_the_specials_are_there():
    x = Q.repeated_world()
    assert (x[:, :, 1:] == x[:, :, :-1]).mean() >= 0.5
    ref = Q.reference(x)
    assert (ref.lower == ref.upper).any()                             # a rank pair inside a run of equal values ...
    assert ((ref.lower != ref.upper) & (ref.q != ref.lower)).any()      # ... and one that interpolates
    s = Q.specials()
    p0 = Q.draws(s, 0)
    for v in (np.inf, -np.inf, Q.SUBNORMAL, -Q.SUBNORMAL):
        assert (p0 == v).sum() >= 1
    assert (np.signbit(p0) & (p0 == 0)).sum() >= 2 and (~np.signbit(p0) & (p0 == 0)).sum() >= 2
    r = Q.reference(s)
    assert r.lower[0, 0] == -np.inf and r.upper[0, -1] == np.inf and np.isnan(r.q[0]).sum() == 0
    assert (Q.draws(s, 1) == s[50, 1, 0]).sum() >= 15 * 9
    assert not np.isnan(s).any() and np.isnan(Q.with_nan(True)).sum() == 1 and np.signbit(Q.with_nan(True)[33, 1, 5])
    # the array worlds reach what they are for: a chain block that is not full, several time chunks, one chain
    assert 257 % 64 and 8200 > 16 * 64 and Q.ARRAY_WORLDS[3][0] == 1


# ---- (e) the surface -----------------------------------------------------------------------------------------------------------------
NEW = ["demcz_quantile_plan", "demcz_select_counts", "demcz_select_step", "demcz_quantile_finish", "demcz_quantiles",
       "demcz_quantiles_array", "demcz_best", "demcz_best_array"]


def test_new_symbols_are_declared_bound_and_exported(demc):
    import ctypes
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "demcz.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(demc.LIB_PATH))
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in demc.SYMBOLS and hasattr(lib, name), name
    jl = (ROOT / "julia" / "DEMCHip.jl").read_text()
    for name in ("demcz_quantiles", "demcz_quantiles_array", "demcz_best", "demcz_best_array"):
        assert f"(:{name}, libdemcz)" in jl, name
    for name in ("quantile_chain", "extract_best", "quantiles", "best"):
        assert re.search(rf"function {name}\(", jl), name
    for name in ("quantile_chain", "extract_best", "posterior_summary", "Quantiles", "Best", "select_step", "quantile_plan", "quantile_finish"):
        assert hasattr(demc, name), name
    for name in ("select_counts", "quantiles", "best"):
        assert hasattr(demc.HipEngine, name) and (name == "select_counts" or hasattr(demc.sampler._Runner, name)), name


# ---- the finishers as a stand-alone program under the sanitizers -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("select_host") / "select_host_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", str(ROOT / "tests" / "c_abi" / "select_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("w", [(257, 20, 40), (1, 5, 4), "low_byte", "repeated", "one_draw", "specials", "nan"], ids=wid)
def test_the_finishers_under_the_sanitizers(sanitized_program, tmp_path, w):
    chain = Q.with_nan(True) if w == "nan" else chain_of(w)
    N, d, G = chain.shape
    ref = Q.reference(chain)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([N * G, d, len(Q.PROBS)], dtype=np.int64).tobytes())
        f.write(np.array(Q.PROBS, dtype=np.float64).tobytes())
        for p in range(d):
            f.write(Q.draws(chain, p).tobytes())
    r = subprocess.run([str(sanitized_program), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = np.array([[int(v, 16) for v in line.split()] for line in r.stdout.splitlines()], dtype=np.uint64).reshape(d, len(Q.PROBS), 3)
    assert np.array_equal(got[:, :, 1], Q.bits(ref.lower)) and np.array_equal(got[:, :, 2], Q.bits(ref.upper))
    assert np.array_equal(got[:, :, 0].view(np.float64), ref.q, equal_nan=True)


def test_the_program_reports_a_rejected_probability(sanitized_program, tmp_path):
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([4, 1, 1], dtype=np.int64).tobytes() + np.array([1.5, 1.0, 2.0, 3.0, 4.0]).tobytes())
    r = subprocess.run([str(sanitized_program), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 4 and "demcz_quantile_plan" in r.stderr
