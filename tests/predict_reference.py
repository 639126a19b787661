"""The random stream of a draw restated in NumPy, for the predictive programs of tests/predict_cases.py.

  * ``philox_blocks``: Philox4x32-10 on uint32 arrays -- block b of the stream (seed, S = (g << 32) | c), what
    ``oracle_py.draw_block(seed, S, b)`` returns, for whole arrays of (g, c, b) at once.
  * ``Streams``: one stream per draw with the consumption rules of the specification -- a block counter from 0, one spare word
    (``uniform``), one spare normal (``normal``), independent of each other; ``bits`` touches neither.  Every method takes a
    ``mask``: the lanes that make the call (the others keep their state), so that divergent programs can be restated.
  * ``u_open`` is exact integer-to-double arithmetic; the Box-Muller pair and dm_log are the oracle's own, element by element.

Everything here is integer arithmetic, exactly representable conversions, or a call of the oracle: the comparison with the device is
bit for bit, and no tolerance appears."""
import numpy as np

import oracle_py

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox_blocks(seed, g, c, b):
    """(r1, r2), uint64 arrays: block ``b`` of the stream of key ``seed`` and subsequence (g << 32) | c, element by element."""
    g, c, b = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(c, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    c0, c1, c2, c3 = b & LOW, b >> S32, c & LOW, g & LOW
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0 | (c1 << S32), c2 | (c3 << S32)


def u_open(r):
    """((r >> 12) + 0.5) * 2^-52: a 52-bit integer, its half-odd successor and a power-of-two scaling, all exact."""
    return ((np.asarray(r, dtype=np.uint64) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def word_to_unit(r):
    """(double)(r >> 11) * 2^-53 in [0, 1), exact: how the test programs turn raw bits into a double."""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def normal_pairs(r1, r2):
    """The oracle's Box-Muller pair of every (r1, r2)."""
    z0, z1 = np.empty(r1.shape), np.empty(r1.shape)
    for i, (a, b) in enumerate(zip(r1.ravel().tolist(), r2.ravel().tolist())):
        z0.flat[i], z1.flat[i] = oracle_py.normal_pair(a, b)
    return z0, z1


class Streams:
    """The streams of the draws (g[i], c[i]) under one seed, each at block 0 with no spare held."""

    def __init__(self, seed, g, c):
        self.seed = int(seed)
        self.g, self.c = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(c, dtype=np.uint64))
        shape = self.g.shape
        self.b = np.zeros(shape, dtype=np.uint64)
        self.spare_word = np.zeros(shape, dtype=np.uint64)
        self.spare_normal = np.zeros(shape)
        self.has_word = np.zeros(shape, dtype=bool)
        self.has_normal = np.zeros(shape, dtype=bool)

    def _mask(self, mask):
        return np.ones(self.g.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)

    def _take(self, take):
        """The next block of the lanes in ``take`` (zeros elsewhere); their counters advance."""
        r1, r2 = np.zeros(self.g.shape, dtype=np.uint64), np.zeros(self.g.shape, dtype=np.uint64)
        if take.any():
            r1[take], r2[take] = philox_blocks(self.seed, self.g[take], self.c[take], self.b[take])
            self.b = self.b + take.astype(np.uint64)
        return r1, r2

    def bits(self, mask=None):
        return self._take(self._mask(mask))

    def uniform(self, mask=None):
        mask = self._mask(mask)
        use, take = mask & self.has_word, mask & ~self.has_word
        r1, r2 = self._take(take)
        out = np.where(use, u_open(self.spare_word), u_open(r1))
        self.spare_word = np.where(take, r2, self.spare_word)
        self.has_word = np.where(take, True, np.where(use, False, self.has_word))
        return out

    def normal(self, mask=None):
        mask = self._mask(mask)
        use, take = mask & self.has_normal, mask & ~self.has_normal
        r1, r2 = self._take(take)
        z0, z1 = np.zeros(self.g.shape), np.zeros(self.g.shape)
        if take.any():
            z0[take], z1[take] = normal_pairs(r1[take], r2[take])
        out = np.where(use, self.spare_normal, z0)
        self.spare_normal = np.where(take, z1, self.spare_normal)
        self.has_normal = np.where(take, True, np.where(use, False, self.has_normal))
        return out

    def exponential(self, mask=None):
        mask = self._mask(mask)
        u = self.uniform(mask)
        out = np.zeros(self.g.shape)
        if mask.any():
            out[mask] = -oracle_py.dm_log(u[mask])
        return out


def window_streams(seed, N, g_from, g_to, chain_id0=0):
    """The streams of the N x w draws of generations g_from..g_to of chains chain_id0 .. chain_id0 + N - 1, as (N, w) arrays."""
    g = np.arange(g_from, g_to + 1, dtype=np.uint64)[None, :]
    c = np.arange(chain_id0, chain_id0 + N, dtype=np.uint64)[:, None]
    return Streams(seed, *np.broadcast_arrays(g, c))


def ppc_counts(values, observed=None):
    """(gt, eq, nan) of an N x m x w array of predicted values against ``observed`` (m values; None: zeros): NumPy's own counts."""
    N, m, w = values.shape
    obs = np.zeros(m) if observed is None else np.asarray(observed, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        gt = np.array([(values[:, k, :] > obs[k]).sum() for k in range(m)], dtype=np.int64)
        eq = np.array([(values[:, k, :] == obs[k]).sum() for k in range(m)], dtype=np.int64)
    nan = np.array([np.isnan(values[:, k, :]).sum() for k in range(m)], dtype=np.int64)
    return gt, eq, nan
