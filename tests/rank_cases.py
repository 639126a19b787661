"""The worlds of the rank tests, shared by test_rank_reference.py (no GPU: every world's conditions are checked there by the
reference alone) and test_gpu_rank.py (the sort, the rank-and-score kernel, the indicator kernel and the calls around them).

The tile of the sort is 1024 keys (RANK_TILE, demcz_kernels_rank.h), a workgroup has 256 lanes, a wave 64."""
import functools

import numpy as np

import stats_cases as S

TILE = 1024
# (N, d, G): less than one wave and odd everything; N no multiple of 64 and many tiles with a ragged last one; more tiles than a
# workgroup has lanes
ARRAY_WORLDS = [(5, 3, 7), (67, 2, 301), (1024, 1, 257)]

# a real run with long runs of exact ties inside the chains: gamma is the knob that brings the acceptance below 30 %
RUN = dict(d=3, N=64, G=200, K=10, gamma=7.0, seed=77)


def ids(w):
    return "x".join(str(v) for v in w) if isinstance(w, tuple) else str(w)


def _frozen(x):
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def all_equal():
    """(67, 2, 9): parameter 0 is one value everywhere, parameter 1 varies."""
    x = np.array(S.world(67, 2, 9), order="F")
    x[:, 0, :] = 1000000.25
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def low_byte():
    """(70, 2, 20): the draws of a parameter differ in the lowest byte of their bit pattern only (parameter 1 negative): seven
    digits are constant, the lowest decides -- and repeats, S = 1400 draws over 256 values."""
    rng = np.random.default_rng(21)
    b = rng.integers(0, 256, size=(70, 2, 20)).astype(np.uint64)
    b[:, 0, :] |= np.uint64(0x3FF0000000000100)
    b[:, 1, :] |= np.uint64(0xC08F400000000000)
    return _frozen(b.view(np.float64))


@functools.lru_cache(maxsize=None)
def sign_only():
    """(33, 1, 40): +-2.5, the keys differ in their top bit (and, being complements, in every digit)."""
    rng = np.random.default_rng(22)
    return _frozen(np.where(rng.random((33, 1, 40)) < 0.4, -2.5, 2.5))


@functools.lru_cache(maxsize=None)
def high_byte_only():
    """(40, 1, 30): 2^k for k in {-600, -344, -88, 168, 424}: the bit patterns differ in the exponent's upper bits alone, so the
    seven lower digits of the keys are constant and only the top digit is sorted by."""
    rng = np.random.default_rng(23)
    k = rng.choice([-600, -344, -88, 168, 424], size=(40, 1, 30))
    return _frozen(np.ldexp(1.0, k))


@functools.lru_cache(maxsize=None)
def specials():
    """(65, 2, 40): normal draws salted with subnormals of both signs, +-0.0 mixed (many of each), +-inf; parameter 1 holds
    values whose keys differ in every digit."""
    rng = np.random.default_rng(24)
    x = rng.standard_normal((65, 2, 40))
    salt = [0.0, -0.0] * 20 + [np.inf, -np.inf] * 3 + [5e-324, -5e-324, 2.0 ** -1040, -(2.0 ** -1040)] * 2
    at = rng.choice(65 * 40, size=len(salt), replace=False)
    for v, i in zip(salt, at):
        x[i % 65, 0, i // 65] = v
    return _frozen(x)


def with_nan(negative=False):
    """(65, 3, 40): specials() with a third parameter, and one NaN in parameter 1."""
    return _nan_pair(negative)[1]


def without_nan():
    return _nan_pair(False)[0]


@functools.lru_cache(maxsize=None)
def _nan_pair(negative):
    rng = np.random.default_rng(25)
    clean = np.concatenate([np.asarray(specials()), 1e6 + rng.standard_normal((65, 1, 40))], axis=1)
    bad = np.array(clean, order="F")
    bad[33, 1, 5] = np.array([0xFFF8000000000000 if negative else 0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    return _frozen(clean), _frozen(bad)


@functools.lru_cache(maxsize=None)
def lattice():
    """(67, 2, 50): draws on a lattice of quarters around a centre that is itself a lattice point: folded at CENTER many draws give
    fabs(0) (of x == center) and every other distance is shared by the two sides."""
    rng = np.random.default_rng(26)
    x = np.empty((67, 2, 50))
    x[:, 0, :] = 3.0 + 0.25 * rng.integers(-8, 9, size=(67, 50))
    x[:, 1, :] = -0.75 + 0.25 * rng.integers(-40, 41, size=(67, 50))
    return _frozen(x)


LATTICE_CENTER = np.array([3.0, -0.75])


# ---- the worlds of the statistic itself ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def independent_normal(N=64, d=2, G=200, seed=31):
    return _frozen(np.random.default_rng(seed).standard_normal((N, d, G)))


@functools.lru_cache(maxsize=None)
def scale_mixture(N=64, d=2, G=200, seed=32):
    """Half the chains have three times the scale of the others and the same mean: what the plain split R-hat cannot see."""
    x = np.random.default_rng(seed).standard_normal((N, d, G))
    x[N // 2:] *= 3.0
    return _frozen(x)


def tile_count(w):
    N, _, G = w
    return -(-N * G // TILE)
