"""The random stream of a draw, CPU tier: the NumPy restatement of tests/predict_reference.py against the
oracle's own Philox, the pinned values of the specification, and the properties the divergent case of tests/predict_cases.py must
have for test_gpu_predict.py to mean what it says."""
import numpy as np

import oracle_py
import predict_cases as pc
import predict_reference as pr

SEED = 20240611


def _S(g, c):
    return (g << 32) | c


def test_numpy_philox_is_the_oracles_draw_block():
    r = np.random.default_rng(1)
    g = np.concatenate([[0, 0, 1, 1, 3, 2**32 - 1, 2**32 - 1], r.integers(0, 2**32, 40)]).astype(np.uint64)
    c = np.concatenate([[0, 5, 0, 2**32 - 1, 2, 0, 2**32 - 1], r.integers(0, 2**32, 40)]).astype(np.uint64)
    b = np.concatenate([[0, 1, 0, 7, 1, 2**32, 2**63], r.integers(0, 2**40, 40)]).astype(np.uint64)
    assert (g == 0).any() and (g >= 1).any() and (b > 0).any()         # S below and from 2^32 on, later blocks
    for seed in (SEED, 0, 2**64 - 1, 0x123456789ABCDEF0):
        r1, r2 = pr.philox_blocks(seed, g, c, b)
        for i in range(g.size):
            assert (int(r1[i]), int(r2[i])) == oracle_py.draw_block(seed, _S(int(g[i]), int(c[i])), int(b[i])), (seed, i)


def test_pinned_blocks():
    assert oracle_py.draw_block(SEED, _S(1, 0), 0) == (0x651BDF940EDD8611, 0xF9F51F10F9878480)
    assert oracle_py.draw_block(SEED, _S(3, 2), 1) == (0xAE1E5CB7D821452B, 0x97739F4DF7075929)
    r1, r2 = pr.philox_blocks(SEED, [1, 3], [0, 2], [0, 1])
    assert [int(v) for v in r1] == [0x651BDF940EDD8611, 0xAE1E5CB7D821452B]
    assert [int(v) for v in r2] == [0xF9F51F10F9878480, 0x97739F4DF7075929]


def test_pinned_uniforms_and_normals():
    s = pr.Streams(SEED, [3], [2])
    assert [float(s.uniform()[0]).hex(), float(s.uniform()[0]).hex()] == ["0x1.2f463e807b791p-1", "0x1.b0884b2928905p-1"]
    assert int(s.b[0]) == 1 and not s.has_word[0]                       # one block: r1, then the spare r2
    s = pr.Streams(SEED, [3], [2])
    assert [float(s.normal()[0]).hex(), float(s.normal()[0]).hex()] == ["0x1.25f3b566afc38p-1", "-0x1.b1c4a9029c162p-1"]
    assert int(s.b[0]) == 1 and not s.has_normal[0]


def test_consumption_rules():
    """Block by block against the oracle: the two spares are independent, bits touches neither, exponential is a uniform."""
    g, c = 7, 11
    blk = [oracle_py.draw_block(SEED, _S(g, c), b) for b in range(6)]
    uo = lambda r: float(pr.u_open(np.uint64(r)))
    s = pr.Streams(SEED, [g], [c])
    assert s.uniform()[0] == uo(blk[0][0])                              # block 0, its r2 held
    assert s.normal()[0] == oracle_py.normal_pair(*blk[1])[0]           # block 1, its z1 held
    r1, r2 = s.bits()
    assert (int(r1[0]), int(r2[0])) == blk[2]                           # block 2, both spares still held
    assert s.uniform()[0] == uo(blk[0][1])
    assert s.normal()[0] == oracle_py.normal_pair(*blk[1])[1]
    assert s.exponential()[0] == -float(oracle_py.dm_log(np.array([uo(blk[3][0])]))[0])      # block 3, its r2 held
    assert s.uniform()[0] == uo(blk[3][1])
    assert int(s.b[0]) == 4
    # a masked call leaves the other lanes alone
    s = pr.Streams(SEED, [g, g], [c, c + 1])
    s.uniform(np.array([True, False]))
    assert s.b.tolist() == [1, 0] and s.has_word.tolist() == [True, False]


def test_streams_do_not_depend_on_the_window():
    a = pr.window_streams(SEED, 5, 1, 9).uniform()
    b = pr.window_streams(SEED, 5, 3, 7).uniform()
    assert np.array_equal(a[:, 2:7], b)
    lo, hi = pr.window_streams(SEED, 3, 1, 9).normal(), pr.window_streams(SEED, 2, 1, 9, chain_id0=3).normal()
    assert np.array_equal(np.vstack([lo, hi]), pr.window_streams(SEED, 5, 1, 9).normal())


def test_divergent_case_diverges_and_stays_below_its_cap():
    """Case (b) at seed 20240611, N = 70, G = 5: no draw reaches the cap of 64 (the largest count is 20), more than half of the draws
    loop at least twice (70 %), and the first wave of generation 1 holds lanes with different counts (12 of them)."""
    N, G = 70, 5
    chain = np.zeros((N, 1, G), order="F")
    out = pc.reference(pc.divergent_numpy, chain, None, SEED)
    n, u = out[:, 0, :], out[:, 1, :]
    print(f"[predict] divergent: max count {int(n.max())}, {100 * (n >= 2).mean():.0f} % loop twice or more, "
          f"{len(set(n[:64, 0].tolist()))} different counts in the first wave")
    assert n.max() < pc.DIVERGENT_CAP
    assert (u >= 0.75).all()                                            # (every loop ended on its own condition)
    assert (n >= 2).mean() > 0.5
    assert len(set(n[:64, 0].tolist())) >= 2


def test_ppc_counts_are_numpys():
    v = np.empty((2, 3, 1), order="F")
    v[0, :, 0], v[1, :, 0] = [1.0, np.nan, np.inf], [0.0, -0.0, -np.inf]
    gt, eq, nan = pr.ppc_counts(v, [0.0, 0.0, np.inf])
    assert gt.tolist() == [1, 0, 0] and eq.tolist() == [1, 1, 1] and nan.tolist() == [0, 1, 0]
    gt, eq, nan = pr.ppc_counts(v, [np.nan, 0.0, 0.0])
    assert gt.tolist() == [0, 0, 1] and eq.tolist() == [0, 1, 0]
