"""Inputs and the reference shared by test_quantile_reference.py (no GPU: the reference, the host finishers of the library, and the
preconditions that give the GPU cases their meaning) and test_gpu_quantiles.py (the counting kernel, demcz_quantiles, demcz_best and
their Python faces).  The reference sorts the order-preserving uint64 keys of the draws and applies the
Hyndman-Fan type 7 formula in NumPy float64, one rounded operation at a time; the best draw is the reference's column-major
findn(bestval .== log_obj)[1] (src/utils.jl:120-125)."""
import functools
from collections import namedtuple

import numpy as np

import stats_cases as S

PROBS = (0.0, 0.025, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.975, 1.0)
ARRAY_WORLDS = [(257, 20, 40), (3, 2, 8200), (600, 9, 20), (1, 5, 4), (64, 3, 260)]
HOT_WORLD, HOT_PARAMETER = (257, 20, 40), 1          # offset 1e6, sd 1: one bin holds every draw in the first three passes

SIGN = np.uint64(1) << np.uint64(63)

Ref = namedtuple("Ref", "q lower upper")


def ids(w):
    return "x".join(str(v) for v in w)


# ---- the order ---------------------------------------------------------------------------------------------------------------------
def keys(x):
    """uint64 keys of float64 values: bits ^ 0xFFFF...F when the sign bit is set, bits | 1 << 63 otherwise."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def from_keys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k ^ SIGN, ~k).view(np.float64)


def draws(chain, p):
    """The S = N G draws of parameter p."""
    return np.ascontiguousarray(chain[:, p, :]).ravel()


# ---- the quantile ------------------------------------------------------------------------------------------------------------------
def plan(S_, probs):
    """(rank_lo, rank_hi, frac) per probability: h = (double)(S-1) q, lo = floor(h) clipped, hi = min(lo+1, S-1), frac = h - lo."""
    lo, hi, frac = [], [], []
    for q in probs:
        h = float(S_ - 1) * float(q)
        l = min(max(int(np.floor(h)), 0), S_ - 1)
        lo.append(l)
        hi.append(min(l + 1, S_ - 1))
        frac.append(h - float(l))
    return np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64), np.array(frac)


def combine(a, b, frac):
    """a when frac == 0 or a == b, else a + frac (b - a), each operation rounded; whatever IEEE gives for infinite a / b."""
    if frac == 0.0 or a == b:
        return a
    with np.errstate(all="ignore"):
        return np.float64(a) + np.float64(frac) * (np.float64(b) - np.float64(a))


def reference(chain, probs=PROBS):
    """Ref(q, lower, upper), each d x nq.  A parameter that holds a NaN is NaN in all three."""
    chain = np.asarray(chain)
    N, d, G = chain.shape
    lo, hi, frac = plan(N * G, probs)
    out = Ref(*(np.empty((d, len(probs)), order="F") for _ in range(3)))
    for p in range(d):
        x = draws(chain, p)
        if np.isnan(x).any():
            for a in out:
                a[p] = np.nan
            continue
        sk = np.sort(keys(x))
        out.lower[p], out.upper[p] = from_keys(sk[lo]), from_keys(sk[hi])
        out.q[p] = [combine(a, b, f) for a, b, f in zip(out.lower[p], out.upper[p], frac)]
    return out


_REFS = {}


def world_reference(w):
    """The reference of stats_cases.world(*w) at PROBS, computed once."""
    if w not in _REFS:
        _REFS[w] = reference(S.world(*w))
    return _REFS[w]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, ref):
    """lower / upper as uint64 views, q with equal_nan: no tolerance."""
    return (np.array_equal(bits(got.lower), bits(ref.lower)) and np.array_equal(bits(got.upper), bits(ref.upper))
            and np.array_equal(got.q, ref.q, equal_nan=True))


# ---- worlds beyond stats_cases -----------------------------------------------------------------------------------------------------
SUBNORMAL = 5e-324


@functools.lru_cache(maxsize=None)
def specials():
    """(65, 3, 9): parameter 0 salted with +-0.0, +-inf and subnormals, parameter 1 with runs of duplicates along time and across
    chains (ranks that fall inside a run of equal values), parameter 2 as it was (offset -3e5)."""
    x = np.array(S.world(65, 3, 9), order="F")
    salt = [0.0, -0.0, np.inf, -np.inf, SUBNORMAL, -SUBNORMAL, 2.0 ** -1040, -(2.0 ** -1040), 0.0, -0.0, np.inf, -np.inf]
    rng = np.random.default_rng(11)
    at = rng.choice(65 * 9, size=len(salt), replace=False)
    for v, i in zip(salt, at):
        x[i % 65, 0, i // 65] = v
    x[10:40, 1, 2:8] = x[10:40, 1, 1:2]             # thirty chains that hold their value for seven generations
    x[50:65, 1, :] = x[50, 1, 0]                     # fifteen chains x nine generations of one value
    x.setflags(write=False)
    return x


def with_nan(negative):
    """specials() with one NaN of the given sign in parameter 1 (not the first draw)."""
    x = np.array(specials(), order="F")
    x[33, 1, 5] = np.array([0xFFF8000000000000 if negative else 0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    return x


@functools.lru_cache(maxsize=None)
def low_byte_world():
    """(70, 2, 5): the draws of a parameter differ only in the lowest byte of their bit pattern (parameter 1 negative): the first
    seven passes see one bin, the last decides everything."""
    rng = np.random.default_rng(12)
    b = rng.integers(0, 256, size=(70, 2, 5)).astype(np.uint64)
    b[:, 0, :] |= np.uint64(0x3FF0000000000100)
    b[:, 1, :] |= np.uint64(0xC08F400000000000)
    x = np.asfortranarray(b.view(np.float64))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def repeated_world():
    """(65, 2, 40): chains that reject repeat their value (chain c keeps it with probability 0.25 + 0.75 c / 64), as a sampled
    history does; parameter 1 is the same walk at offset 1e6."""
    rng = np.random.default_rng(13)
    keep_p = 0.25 + 0.75 * np.arange(65) / 64
    v = np.empty((65, 40))
    v[:, 0] = rng.standard_normal(65)
    for g in range(1, 40):
        v[:, g] = np.where(rng.random(65) < keep_p, v[:, g - 1], rng.standard_normal(65))
    x = np.asfortranarray(np.stack([v, 1e6 - 3.0 * v], axis=1))
    x.setflags(write=False)
    return x


def one_draw():
    return np.asfortranarray(np.full((1, 1, 1), -2.5))


# ---- the counting pass in NumPy ----------------------------------------------------------------------------------------------------
def count_pass(chain, shift, prefix):
    """What demcz_select_counts returns: (counts (d, nprefix, 256) int64, nan_count (d,)).  At shift 56 every draw matches every
    prefix; below, a draw counts towards the first prefix that equals key >> (shift + 8)."""
    chain = np.asarray(chain)
    d = chain.shape[1]
    prefix = np.asarray(prefix, dtype=np.uint64).reshape(d, -1)
    counts = np.zeros((d, prefix.shape[1], 256), dtype=np.int64)
    nan = np.zeros(d, dtype=np.int64)
    for p in range(d):
        x = draws(chain, p)
        k = keys(x)
        nan[p] = int(np.isnan(x).sum())
        digit = ((k >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        taken = np.zeros(k.shape, dtype=bool)
        for u in range(prefix.shape[1]):
            if shift == 56:
                m = np.ones(k.shape, dtype=bool)
            else:
                m = ((k >> np.uint64(shift + 8)) == prefix[p, u]) & ~taken
                taken |= m
            counts[p, u] = np.bincount(digit[m], minlength=256)
    return counts, nan


def bin_share(chain, p, passes=8):
    """Per pass of a selection that follows the median: the largest share of the draws still in play that falls into one bin."""
    k = keys(draws(chain, p))
    rank, out = (k.size - 1) // 2, []
    for i in range(passes):
        shift = 56 - 8 * i
        c = np.bincount(((k >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        out.append(c.max() / k.size)
        b = int(np.searchsorted(np.cumsum(c), rank, side="right"))
        rank -= int(c[:b].sum())
        k = k[((k >> np.uint64(shift)) & np.uint64(255)) == np.uint64(b)]
    return out


# ---- the best draw -----------------------------------------------------------------------------------------------------------------
def best_reference(log_obj):
    """(bestval, chain, column), 0-based: the maximum ignoring NaN; ties by == go to the earliest column, then the lowest chain."""
    lo = np.asarray(log_obj)
    if np.isnan(lo).all():
        return np.nan, -1, -1
    v = np.nanmax(lo)
    g, c = np.argwhere((lo == v).T)[0]
    return float(v), int(c), int(g)
