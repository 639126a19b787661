"""CPU tier of the posterior densities (no GPU): the references of tests/density_cases.py against NumPy's own histograms and the
plain HDI formula; the host half of the library (demcz_density_host.h: the edge table, the bin placement the kernels compile,
the HDI's step count and the pair-tile plan), walked by a stand-alone program built under AddressSanitizer and UBSan
(tests/c_abi/density_host_main.cpp) and held to the references and to the library's own exports of the same text; and the
conditions that give the GPU cases of test_gpu_density.py their meaning, checked on the references alone."""
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import density_cases as D
import quantile_cases as Q
import stats_cases as S

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("density_host")
    exe = tmp / "density_host_main"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", str(ROOT / "tests" / "c_abi" / "density_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find|libasan|libubsan|asan_rt|ubsan_standalone", r.stderr):
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    count = [0]

    def run(mode, payload):
        count[0] += 1
        path = tmp / f"{mode}{count[0]}.in"
        if isinstance(payload, bytes):
            path.write_bytes(payload)
        else:
            path.write_text(payload)
        p = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:], p.stdout[-500:])
        return p.stdout.splitlines()

    return run


FINITE_WORLDS = [w for w in D.WORLDS if w != (1, 1, 1)] + [(65, 3, 9)]


# ---- the references against NumPy's own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", FINITE_WORLDS, ids=D.ids)
def test_reference_counts_are_numpys_histogram(w):
    chain = S.world(*w)
    for nb in D.NBINS:
        ref = D.hist_reference(chain, nb)
        assert not ref.below.any() and not ref.above.any() and not ref.nan.any()
        for p in range(w[1]):
            c, e = np.histogram(D.draws(chain, p), bins=nb, range=tuple(D.auto_range(chain)[p]))
            assert np.array_equal(c, ref.counts[p]) and np.array_equal(D.bits(e), D.bits(ref.edges[p])), (nb, p)
    lo, hi = np.percentile(chain, [20, 70], axis=(0, 2))                  # a given range with draws on either side of it
    ref = D.hist_reference(chain, 33, np.stack([lo, hi], axis=1))
    for p in range(w[1]):
        x = D.draws(chain, p)
        assert np.array_equal(np.histogram(x, bins=33, range=(lo[p], hi[p]))[0], ref.counts[p])
        assert ref.below[p] == (x < lo[p]).sum() and ref.above[p] == (x > hi[p]).sum()
        assert ref.counts[p].sum() + ref.below[p] + ref.above[p] == x.size


def test_reference_of_one_draw_and_of_a_constant_parameter():
    one = D.hist_reference(S.world(1, 1, 1), 33)
    assert one.counts.sum() == 1 and one.counts[0, 16] == 1               # numpy's (x - 0.5, x + 0.5): the middle bin
    chain = D.constant_world()
    ref = D.hist_reference(chain, 33)
    assert np.array_equal(ref.edges[1][[0, -1]], [1000000.25 - 0.5, 1000000.25 + 0.5]) and ref.counts[1, 16] == 65 * 4
    assert np.array_equal(np.histogram(D.draws(chain, 1), bins=33)[0], ref.counts[1])


@pytest.mark.parametrize("w", [(63, 2, 5), (65, 9, 7), (3, 2, 2051)], ids=D.ids)
def test_reference_pairs_are_numpys_histogram2d(w):
    chain = S.world(*w)
    d = w[1]
    pairs = [(p, q) for p in range(d) for q in range(d) if p != q][:12]
    r = D.auto_range(chain)
    for nbx, nby in D.GRIDS:
        ref = D.hist2d_reference(chain, pairs, nbx, nby)
        assert not ref.outside.any()
        for i, (p, q) in enumerate(pairs):
            want = np.histogram2d(D.draws(chain, p), D.draws(chain, q),
                                  bins=[D.edges_of(*r[p], nbx), D.edges_of(*r[q], nby)])[0]
            assert np.array_equal(want.astype(np.int64), ref.counts[i]), (nbx, nby, p, q)


def test_hdi_reference_is_the_plain_formula_on_tie_free_worlds():
    for w in [(63, 2, 5), (65, 9, 7), (257, 20, 3), (3, 2, 2051)]:
        chain = S.world(*w)
        ref = D.hdi_reference(chain, D.HDI_PROBS)
        for p in range(w[1]):
            x = D.draws(chain, p)
            assert np.unique(x).size == x.size
            for j, prob in enumerate(D.HDI_PROBS):
                _, m, wd = D.hdi_widths(x, prob)
                if np.unique(wd).size == wd.size:                          # (no two starts of one width)
                    assert tuple(ref[p, j]) == D.hdi_plain(x, prob), (w, p, prob)
                assert m == min(int(prob * x.size), x.size - 1)


def test_multimodal_hdi_of_two_modes():
    counts = np.array([[0, 5, 9, 5, 0, 0, 4, 8, 4, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1]], dtype=np.int64)
    edges = np.stack([np.linspace(0.0, 10.0, 11), np.linspace(-1.0, 1.0, 11)])
    got = D.multimodal_reference(counts, edges, 0.8)                       # 9 + 8 + 5 + 5 = 27 < 0.8 * 35 = 28 <= 27 + 4
    assert got[0] == [(1.0, 4.0), (6.0, 8.0)]
    assert got[1] == [(-1.0, edges[1][8])]                                 # ties: rising index, 8 of 10 bins reach 0.8
    assert D.multimodal_reference(counts, edges, 0.2)[0] == [(2.0, 3.0)]   # 9 >= 0.2 * 35: the fullest bin alone


# ---- the host half of the library ------------------------------------------------------------------------------------------------------
RANGES = [(0.0, 1.0), (-1.0, 1.0), (0.0, 3.3), (-0.7, 0.1), (1e6 - 4.0, 1e6 + 5.0), (-3e5, -3e5 + 1e-3), (5e-324, 1e-320),
          (-1e308, 1e307), (1.0, np.nextafter(1.0, 2.0)), (1e16, 1e16 + 2.0), (-0.0, 7.0)]


def test_edge_tables_are_linspace(host, demc):
    refused = 0
    for lo, hi in RANGES:
        for nb in D.NBINS + (3, 7, 1000):
            want = np.linspace(lo, hi, nb + 1)
            if (np.diff(want) < 0).any():                                 # a span of a few subnormals: refused, not mis-binned
                assert hi < 1e-300 and host("place", struct.pack("qqdd", nb, 0, lo, hi)) == ["refused 1"]
                refused += 1
                continue
            got = demc.histogram_edges(nb, lo, hi)
            assert np.array_equal(D.bits(got), D.bits(want)), (lo, hi, nb)
            line = host("place", struct.pack("qqdd", nb, 0, lo, hi))[0]
            assert np.array_equal(np.array([int(h, 16) for h in line.split()], dtype=np.uint64), D.bits(want)), (lo, hi, nb)
    assert refused >= 1
    for nb, lo, hi in [(0, 0.0, 1.0), (4097, 0.0, 1.0), (33, 1.0, 1.0), (33, 2.0, 1.0), (33, np.nan, 1.0), (33, 0.0, np.inf),
                       (33, -1e308, 1e308)]:
        with pytest.raises(demc.DemczError) as ei:
            demc.histogram_edges(nb, lo, hi)
        assert ei.value.code == 1
        assert host("place", struct.pack("qqdd", nb, 0, lo, hi)) == ["refused 1"]


def test_the_placement_the_kernels_compile_is_the_references(host):
    """density_bin -- the estimate and the bounded walk along the table -- on draws on, one ulp below and one ulp above every edge,
    on random draws in and out of range, and on the special values, over ranges where the estimate's rounding matters."""
    gen = np.random.default_rng(16)
    for lo, hi in RANGES:
        for nb in (1, 2, 33, 256, 4096, 1000):
            e = np.linspace(lo, hi, nb + 1)
            if (np.diff(e) < 0).any():
                continue
            x = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), gen.uniform(lo, hi, 500),
                                lo + (hi - lo) * gen.uniform(-0.5, 1.5, 200),
                                [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.0 ** -1040]])
            out = host("place", struct.pack("qqdd", nb, x.size, lo, hi) + x.tobytes())
            got = np.array([int(v) for v in out[1:]])
            want = D.place(x, e)
            want = np.where(want == -1, nb, np.where(want == -2, nb + 1, np.where(want == -3, nb + 2, want)))
            assert np.array_equal(got, want), (lo, hi, nb)


def test_hdi_steps(host, demc):
    cases = [(S_, prob) for S_ in (1, 2, 3, 585, 10 ** 6, 2 ** 31 - 1)
             for prob in (0.94, 0.5, 1e-12, 5e-324, np.nextafter(1.0, 0.0), 1.0 / 3.0, 0.999)]
    out = host("steps", "".join(f"{S_} {struct.unpack('Q', struct.pack('d', prob))[0]:x}\n" for S_, prob in cases))
    for (S_, prob), line in zip(cases, out):
        rc, m = (int(v) for v in line.split())
        assert rc == 0 and m == D.hdi_steps(S_, prob) == int(demc.hdi_steps(S_, prob)[0]) and 0 <= m <= S_ - 1, (S_, prob)
    bad = [0.0, 1.0, np.nan, -0.5, 1.5, np.inf]
    out = host("steps", "".join(f"10 {struct.unpack('Q', struct.pack('d', prob))[0]:x}\n" for prob in bad) + "0 3fe0000000000000\n")
    assert [int(l.split()[0]) for l in out] == [1] * (len(bad) + 1)
    for probs in ([0.0], [1.0], [np.nan], [0.5] * 17, []):
        with pytest.raises(demc.DemczError):
            demc.hdi_steps(10, probs)


def parse_plan(lines, cases):
    """Per case: (cap, a, b, columns_read, tiles), a tile being (nrow, ncol, npair, mask, row, col, col_row, out)."""
    it = iter(lines)
    out = []
    for _ in cases:
        cap, a, b, ntiles, cols = (int(v) for v in next(it).split())
        tiles = []
        for _ in range(ntiles):
            head, row, col, col_row, slots = next(it).split("|")
            nrow, ncol, npair, mask = head.split()
            tiles.append((int(nrow), int(ncol), int(npair), int(mask, 16), [int(v) for v in row.split()], [int(v) for v in col.split()],
                          [int(v) for v in col_row.split()], [int(v) for v in slots.split()]))
        out.append((cap, a, b, cols, tiles))
    return out


def plan_cases():
    gen = np.random.default_rng(17)
    cases = [(9, 32, 32, D.ALL36), (9, 128, 128, D.ALL36), (9, 1, 1, D.ALL36), (9, 32, 17, D.ALL36), (2, 128, 128, [(0, 1)]),
             (2, 32, 32, [(1, 0), (0, 1)]), (4, 32, 32, D.MIXED_PAIRS[:-1]), (20, 32, 32, [(p, q) for p in range(20) for q in range(p + 1, 20)]),
             (33, 8, 8, [(p, q) for p in range(33) for q in range(33) if p != q]), (33, 128, 3, [(32, 0), (0, 32), (5, 6)])]
    for d in (3, 9, 20):
        allp = [(p, q) for p in range(d) for q in range(d) if p != q]
        for nb in ((16, 16), (40, 40), (128, 64), (5, 3)):
            pick = gen.permutation(len(allp))[:int(gen.integers(1, len(allp) + 1))]
            cases.append((d, nb[0], nb[1], [allp[i] for i in pick]))
    return cases


def test_the_pair_tile_plan_covers_every_pair_once_within_the_lds_budget(host):
    cases = plan_cases()
    text = "".join(f"{d} {nbx} {nby} {len(pairs)} " + " ".join(f"{p} {q}" for p, q in pairs) + "\n" for d, nbx, nby, pairs in cases)
    plans = parse_plan(host("plan", text), cases)
    for (d, nbx, nby, pairs), (cap, a, b, cols, tiles) in zip(cases, plans):
        assert cap == min(64, 16384 // (nbx * nby)) and 1 <= a <= 8 and 1 <= b <= 8 and a * b <= cap
        seen, read = {}, 0
        for nrow, ncol, npair, mask, row, col, col_row, slots in tiles:
            assert 1 <= nrow <= a and 1 <= ncol <= b and 1 <= npair <= cap and npair * nbx * nby * 4 <= 65536
            assert all(0 <= v < d for v in row[:nrow] + col[:ncol]) and row[nrow:] == [-1] * (8 - nrow) and col[ncol:] == [-1] * (8 - ncol)
            assert len(set(row[:nrow])) == nrow and len(set(col[:ncol])) == ncol
            bits_set = [bit for bit in range(64) if mask >> bit & 1]
            assert len(bits_set) == npair == len(slots)
            for slot, bit in enumerate(bits_set):                         # the kernel's numbering: slots in bit order
                r, c = divmod(bit, 8)
                assert r < nrow and c < ncol
                pq = (row[r], col[c])
                assert pairs[slots[slot]] == pq and pq not in seen
                seen[pq] = slots[slot]
            for c in range(8):
                assert col_row[c] == (row.index(col[c]) if c < ncol and col[c] in row[:nrow] else -1)
            read += len(set(row[:nrow]) | set(col[:ncol]))
        assert sorted(seen) == sorted(set(pairs)) and sorted(seen.values()) == list(range(len(pairs)))
        assert cols == read <= 2 * len(pairs)
    # the figures DESIGN.md section 4.18 quotes: columns read under the plan against the two per pair of a pair at a time
    by_case = {(c[0], c[1], c[2], len(c[3])): p for c, p in zip(cases, plans)}
    assert (by_case[(9, 32, 32, 36)][3], len(by_case[(9, 32, 32, 36)][4])) == (18, 3)
    assert (by_case[(20, 32, 32, 190)][3], len(by_case[(20, 32, 32, 190)][4])) == (100, 15)
    assert by_case[(9, 128, 128, 36)][3] == 72 and by_case[(9, 1, 1, 36)][3] == 9
    out = host("plan", "0 32 32 1 0 1\n3 129 32 1 0 1\n3 32 0 1 0 1\n")
    assert out == ["refused 1"] * 3


def test_constants_of_the_header():
    text = (ROOT / "demc.jl_amd" / "csrc" / "demcz_density_host.h").read_text()
    for name, value in [("DENSITY_MAX_BINS", 4096), ("DENSITY_MAX_SIDE", 128), ("DENSITY_LDS_CELLS", 16384), ("DENSITY_TILE_SIDE", 8),
                        ("DENSITY_MAX_PROBS", 16)]:
        assert re.search(rf"constexpr int {name} = {value};", text), name


def test_the_exports_are_declared_bound_and_in_the_library(demc):
    import ctypes
    lib = ctypes.CDLL(str(demc.LIB_PATH))
    hdr = (ROOT / "include" / "demcz.h").read_text()
    jl = (ROOT / "julia" / "DEMCHip.jl").read_text()
    for name in ("demcz_histogram_edges", "demcz_histogram", "demcz_histogram_array", "demcz_histogram2d", "demcz_histogram2d_array",
                 "demcz_hdi_steps", "demcz_hdi", "demcz_hdi_array"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in demc.SYMBOLS and hasattr(lib, name), name
    for name in ("demcz_histogram", "demcz_histogram2d", "demcz_hdi"):
        assert re.search(rf"ccall\(\(:{name},", jl), name


def test_histogram_record(demc):
    """Histogram.density, .mode and .hdi (host code) on counts made here."""
    counts = np.array([[0, 5, 9, 5, 0, 0, 4, 8, 4, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [0] * 10], dtype=np.int64)
    edges = np.stack([np.linspace(0.0, 10.0, 11), np.linspace(-1.0, 1.0, 11), np.linspace(0.0, 1.0, 11)])
    z = np.zeros(3, dtype=np.int64)
    h = demc.Histogram(counts, edges, z, z, z)
    assert np.array_equal(h.density[0], counts[0] / (35 * np.diff(edges[0])))
    assert np.allclose((h.density[:2] * np.diff(edges[:2], axis=1)).sum(axis=1), 1.0) and np.isnan(h.density[2]).all()
    assert np.array_equal(h.mode()[:2], [2.5, 0.5 * (edges[1, 0] + edges[1, 1])])
    for prob in (0.2, 0.5, 0.8, 0.94, 0.999):
        assert h.hdi(prob) == D.multimodal_reference(counts, edges, prob), prob
    assert h.hdi(0.5)[2] == []
    for bad in (0.0, 1.0, np.nan):
        with pytest.raises(ValueError):
            h.hdi(bad)


# ---- the worlds reach what they are for ------------------------------------------------------------------------------------------------
def test_a_world_has_whole_wave_runs_in_one_bin_and_another_spreads_a_wave_over_many():
    chain, rng = D.piled_world()
    e = D.edges_of(*rng[0], 33)
    nb = D.wave_bins(chain, 0, e)
    runs = (nb.reshape(nb.shape[0], -1, 4) == 1).all(axis=2)              # the four generations a wave loads at a time
    assert runs.mean() > 0.5 and (nb > 1).any()                           # runs that are kept in scalars, and runs that end
    assert (D.wave_bins(chain, 1, D.edges_of(*rng[1], 33)) >= 8).all()
    chain = S.world(*D.SPREAD_WORLD)
    r = D.auto_range(chain)
    for p in (0, 1, 4):                                                   # parameter 1: 1e6 standard deviations from zero
        assert (D.wave_bins(chain, p, D.edges_of(*r[p], 33))[:4] >= 8).all(), p
    assert abs(chain[:, 1, :].mean()) > 0.9e6 * chain[:, 1, :].std()
    ref = D.hist_reference(chain, 33)
    assert (ref.counts[1] > 0).sum() >= 20                                # ... and the automatic range still resolves it


def test_the_out_of_range_world_has_draws_of_every_kind():
    chain, rng = D.out_of_range_world()
    assert np.isinf(chain).any() and (np.abs(chain[chain != 0]) < 2.3e-308).any() and np.signbit(chain[chain == 0]).any()
    nan = np.isnan(chain)
    assert np.signbit(chain[nan]).any() and not np.signbit(chain[nan]).all()
    for nb in (1, 33):
        ref = D.hist_reference(chain, nb, rng)
        assert (ref.below > 0).all() and (ref.above > 0).all() and (ref.nan == 2).all()
        assert (2 * (ref.below + ref.above + ref.nan) < 65 * 9).all()
        assert np.array_equal(ref.counts.sum(axis=1) + ref.below + ref.above + ref.nan, [65 * 9] * 3)
    two = D.hist2d_reference(chain, [(0, 1), (2, 0)], 32, 17, rng)
    assert (two.outside > 0).all() and (two.counts.sum(axis=(1, 2)) + two.outside == 65 * 9).all()


def test_the_edge_worlds_put_draws_on_and_next_to_every_edge():
    for nb in D.NBINS:
        chain, rng = D.edge_world(nb)
        ref = D.hist_reference(chain, nb, rng)
        for p in range(2):
            x, e = D.draws(chain, p), ref.edges[p]
            assert np.isin(e, x).all() and np.isin(np.nextafter(e, -np.inf), x).all() and np.isin(np.nextafter(e, np.inf), x).all()
            assert ref.below[p] >= 1 and ref.above[p] >= 1
            k = D.place(x, e)
            assert (k[x == e[nb]] == nb - 1).all() and (k[x == e[0]] == 0).all()
        x0 = D.draws(chain, 0)
        assert (np.signbit(x0) & (x0 == 0)).any() and ref.edges[0][0] == 0.0     # -0.0 against the edge 0.0: bin 0, not below
        assert (D.place(x0[x0 == 0], ref.edges[0]) == 0).all()


def test_the_hdi_worlds_hold_ties_and_nan_widths():
    chain = D.hdi_special_world()
    s, m, wd = D.hdi_widths(D.draws(chain, 1), 0.2)
    assert m == 117 and (wd == wd.min()).sum() >= 2 and wd.min() == 0.0   # chains that stood still: many starts of width 0
    ref = D.hdi_reference(chain, D.HDI_PROBS)
    assert ref[1, 2, 0] == ref[1, 2, 1] == chain[50, 1, 0]
    s, m, wd = D.hdi_widths(D.draws(chain, 0), 0.001)
    assert m == 0 and np.isnan(wd).any() and not np.isnan(wd).all()       # inf - inf: no candidate, the first finite draw wins
    assert ref[0, 4, 0] == ref[0, 4, 1] == s[np.isfinite(s)][0]
    s, m, wd = D.hdi_widths(D.draws(chain, 0), 0.999)
    assert np.isinf(wd[~np.isnan(wd)]).all() and np.isinf(ref[0, 3]).all()      # an infinite width is a candidate
    both = D.hdi_reference(Q.with_nan(True), D.HDI_PROBS)
    assert np.isnan(both[1]).all() and np.array_equal(D.bits(both[[0, 2]]), D.bits(ref[[0, 2]]))
    allinf = np.full((3, 1, 2), np.inf)
    assert np.isnan(D.hdi_reference(allinf, [0.5])).all()                 # no candidate at all


def test_the_36_pair_world_needs_two_tiles_or_more(host):
    plan = parse_plan(host("plan", "9 32 32 36 " + " ".join(f"{p} {q}" for p, q in D.ALL36) + "\n"), [None])[0]
    assert len(plan[4]) >= 2 and plan[0] == 16
