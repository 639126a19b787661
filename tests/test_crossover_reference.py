"""CPU tier of the crossover generation: the pieces of the reference step (tests/crossover_reference.py) are what DESIGN.md
section 3 says.

  * with every parameter selected and one pair the proposal is the full-block formula x + ((gamma / sqrt(2 d)) (za - zb) + eps z),
    operation by operation in NumPy; with a subset, the unselected parameters keep their bits and the scale is
    gamma / sqrt(2 delta d') -- also at d' = 1, where the reference's full-block step has its b == 1 quirk and this one has none;
  * the selection rule at its edges: word 0 and word 2^32 - 1, the last class selects everything, ncr = 1;
  * the class draw against cumulative weights that contain zeros, and the number of pairs, at the ends of the word;
  * the stride S_cr at d = 2, 4, 5, 8, 9, 64;
  * a step's facts agree with the words of its blocks (the layout of a generation), block by block."""
import numpy as np
import pytest

import crossover_reference as cr

W32 = (1 << 32) - 1


def test_all_selected_and_one_pair_is_the_full_block_formula():
    r = np.random.default_rng(5)
    for d in (2, 5, 7, 20):
        x, za, zb, z, eps = (r.standard_normal(d) for _ in range(5))
        eps = np.abs(eps) * 1e-2
        gamma = 2.38
        xp, scale = cr.proposal([float(v) for v in x], list(range(d)), [(list(za), list(zb))], list(z), gamma, list(eps))
        sc = np.float64(gamma) / np.sqrt(np.float64(2 * d))
        want = x + ((sc * (za - zb)) + (eps * z))
        assert scale == float(sc) and np.array_equal(np.array(xp), want), d


def test_a_subset_leaves_the_other_parameters_their_bits_and_scales_by_its_size():
    r = np.random.default_rng(6)
    d = 9
    x = [float(v) for v in r.standard_normal(d)]
    rows = [([float(v) for v in r.standard_normal(d)], [float(v) for v in r.standard_normal(d)]) for _ in range(3)]
    z = [float(v) for v in r.standard_normal(d)]
    eps = [1e-3] * d
    for sel in ([4], [0, 8], [1, 2, 3, 5, 7]):
        for delta in (1, 2, 3):
            xp, scale = cr.proposal(x, sel, rows[:delta], z, 0.9, eps)
            assert scale == float(np.float64(0.9) / np.sqrt(np.float64(2 * delta * len(sel))))
            for p in range(d):
                if p not in sel:
                    assert xp[p] is x[p] or np.float64(xp[p]).tobytes() == np.float64(x[p]).tobytes()
                else:
                    s = np.float64(rows[0][0][p]) - np.float64(rows[0][1][p])
                    for j in range(1, delta):
                        s = s + (np.float64(rows[j][0][p]) - np.float64(rows[j][1][p]))
                    assert xp[p] == float(np.float64(x[p]) + (np.float64(scale) * s + np.float64(eps[p]) * np.float64(z[p])))
    # d' = 1: gamma / sqrt(2 delta), not the bare gamma of the full-block step's b == 1 quirk
    _, scale = cr.proposal(x, [3], rows[:1], z, 0.9, eps)
    assert scale == float(np.float64(0.9) / np.sqrt(np.float64(2.0))) != 0.9


def test_the_selection_rule_at_its_edges():
    for ncr in range(1, 9):
        for m in range(ncr):
            assert cr.selects(0, ncr, m)                                   # word 0 is selected in every class
            assert cr.selects(W32, ncr, m) == (m == ncr - 1)               # the largest word only where everything is
            # the threshold: word ncr < (m + 1) 2^32, i.e. exactly ceil((m + 1) 2^32 / ncr) words of 2^32
            t = -(-((m + 1) << 32) // ncr)
            assert cr.selects(t - 1, ncr, m) and (t > W32 or not cr.selects(t, ncr, m))
        assert all(cr.selects(w, ncr, ncr - 1) for w in (0, 1, 1 << 31, W32))
    assert all(cr.selects(w, 1, 0) for w in (0, 12345, W32))               # ncr = 1: every parameter, always
    # the probability is (m + 1) / ncr exactly: the count of selecting words
    assert -(-(2 << 32) // 3) == 2863311531 and not cr.selects(2863311531, 3, 1) and cr.selects(2863311530, 3, 1)


def test_the_class_draw_against_weights_with_zeros():
    cum = cr.cumulative([0, 3, 0, 1])
    assert cum == [0, 3, 3, 4]
    assert cr.cr_class(0, cum) == 1 and cr.cr_class(W32, cum) == 3         # never class 0 or 2
    assert cr.cr_class((3 << 30) - 1, cum) == 1 and cr.cr_class(3 << 30, cum) == 3      # j = 2 | 3
    got = [cr.cr_class((k << 32) // 400 + 7, cum) for k in range(400)]
    assert got.count(1) == 300 and got.count(3) == 100 and got == sorted(got)
    cum = cr.cumulative([2, 0, 5])
    assert {cr.cr_class((k << 32) // 70, cum) for k in range(70)} == {0, 2}
    assert [cr.cr_class((k << 32) // 7 + 1, cum) for k in range(7)] == [0, 0, 2, 2, 2, 2, 2]
    assert cr.cr_class(W32, cr.cumulative([1])) == 0
    assert cr.cr_class(W32, cr.cumulative([(1 << 31) - 1])) == 0
    for dm in (1, 2, 3):
        assert cr.n_pairs(0, dm) == 1 and cr.n_pairs(W32, dm) == dm
        assert sorted({cr.n_pairs((k << 32) // 60, dm) for k in range(60)}) == list(range(1, dm + 1))
    assert cr.fallback_parameter(0, 7) == 0 and cr.fallback_parameter((1 << 64) - 1, 7) == 6 and cr.fallback_parameter(1 << 63, 64) == 32


def test_the_stride():
    # 1 + delta_max + ceil(d / 4) + ceil(d / 2) + 1
    assert [cr.stride(d, 3) for d in (2, 4, 5, 8, 9, 64)] == [7, 8, 10, 11, 13, 53]
    assert [cr.stride(d, 1) for d in (2, 4, 5, 8, 9, 64)] == [5, 6, 8, 9, 11, 51]
    assert min(cr.stride(d, dm) for d in range(2, 65) for dm in (1, 2, 3)) == 5          # a snooker generation reads three blocks


@pytest.mark.parametrize("d,ncr,delta_max,weights", [(5, 3, 3, None), (9, 8, 2, None), (33, 3, 3, [2, 0, 5]), (64, 3, 1, None)])
def test_a_step_reads_its_blocks_where_the_spec_puts_them(oracle, d, ncr, delta_max, weights):
    O = oracle
    r = np.random.default_rng(d)
    M, seed = 50, 99
    Z = r.standard_normal((M, d))
    cum = cr.cumulative(weights or [1] * ncr)
    S = cr.stride(d, delta_max)
    seen_fallback = False
    for chain in range(40):
        g = 3 + chain
        B = (g - 1) * S
        x = [float(v) for v in r.standard_normal(d)]
        lp0 = -0.5 * sum(v * v for v in x)
        logobj = lambda q: -0.5 * sum(v * v for v in q)
        xn, lpn, f = cr.crossover_step(O, seed, chain, B, Z, M, x, lp0, logobj, 0.8, [1e-3] * d, ncr, delta_max, cum)
        w = cr.words(*O.draw_block(seed, chain, B))
        assert f["m"] == cr.cr_class(w[1], cum) and f["delta"] == cr.n_pairs(w[0], delta_max)
        assert f["pstar"] == (O.draw_block(seed, chain, B)[1] * d) >> 64
        assert f["pairs"] == [O.draw_rows(seed, chain, B + 1 + j, M) for j in range(delta_max)] and all(a != b for a, b in f["pairs"])
        sel = [p for p in range(d) if cr.selects(cr.words(*O.draw_block(seed, chain, B + 1 + delta_max + p // 4))[p % 4], ncr, f["m"])]
        assert f["fallback"] == (not sel) and f["mask"] == (sum(1 << p for p in sel) or 1 << f["pstar"])
        seen_fallback |= f["fallback"]
        B_n = B + 1 + delta_max + -(-d // 4)
        z = [v for pr in range(-(-d // 2)) for v in O.normal_pair(*O.draw_block(seed, chain, B_n + pr))]
        rows = [([float(v) for v in Z[a]], [float(v) for v in Z[b]]) for a, b in f["pairs"][:f["delta"]]]
        xp, _ = cr.proposal(x, [p for p in range(d) if f["mask"] >> p & 1], rows, z, 0.8, [1e-3] * d)
        assert xp == f["xp"]
        assert f["logu"] == float(O.dm_log(cr.sr.u_open(O.draw_block(seed, chain, B + S - 1)[0])))
        assert (xn == f["xp"] and lpn == f["lp_prop"]) if f["accepted"] else (xn == x and lpn == lp0)
        assert f["accepted"] == (f["logu"] < f["lp_prop"] - lp0)
    assert seen_fallback or d > 5


def test_nan_rejects_and_temperature_divides(oracle):
    O = oracle
    Z = np.random.default_rng(1).standard_normal((20, 4))
    x = [0.1, 0.2, 0.3, 0.4]
    for chain in range(8):
        _, lpn, f = cr.crossover_step(O, 1, chain, 0, Z, 20, x, -1.0, lambda q: float("nan"), 0.8, [1e-3] * 4, 3, 3, [1, 2, 3])
        assert not f["accepted"] and lpn == -1.0
        _, _, f = cr.crossover_step(O, 1, chain, 0, Z, 20, x, -1.0, lambda q: -2.0, 0.8, [1e-3] * 4, 3, 3, [1, 2, 3], T=0.0)
        assert not f["accepted"]                                   # (-1) / 0 = -inf
        _, _, f = cr.crossover_step(O, 1, chain, 0, Z, 20, x, -1.0, lambda q: -0.5, 0.8, [1e-3] * 4, 3, 3, [1, 2, 3], T=0.0)
        assert f["accepted"]                                       # 0.5 / 0 = +inf
