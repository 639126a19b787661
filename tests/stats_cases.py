"""Inputs shared by test_stats_reference.py (which checks, without a GPU, that they and the tolerances mean something) and
test_gpu_stats.py (which runs them through the statistics kernels): seeded chain histories and log_obj histories at the smallest
shapes that reach each edge of K5 / K7a / K7b, and the references of them, computed once (stats_reference.py)."""
import functools

import numpy as np

import stats_reference as R

# ---- worlds: x = A z + a per-chain constant, every parameter then scaled and offset ----------------------------------------------
OFFSETS = (0.0, 1e6, -3e5, 1e3, -1e6, 7.0)
SDS = (1.0, 1.0, 0.25, 1e-3, 4.0, 1e3)          # offset / sd reaches 1.2e6 and no further: beyond that the float64 storage of the
CHAIN_SD = 0.3                                  # split-chain means limits R-hat, in the oracle too

MEANCOV_WORLDS = ([(257, d, 40) for d in (1, 7, 8, 9, 16, 17, 20, 33, 64)]
                  + [(N, 20, 40) for N in (1, 255, 256, 600)]
                  + [(257, 20, G) for G in (1, 2, 16, 17, 100)]
                  + [(3, 2, 8200)])             # 512 chunks of 17 generations: the last 29 are empty
MEANCOV_EXACT = (1, 3, 1)                       # the mean is the sample and the covariance is 0, both exactly
RHAT_WORLDS = [(257, 20, 131), (3, 33, 65), (600, 9, 20), (1, 5, 4), (2, 1, 5), (128, 9, 130), (256, 2, 2051), (300, 3, 4100)]
CONTAMINATED = (257, 20, 40)
POISON_AT = (100, 11, 17)                       # (chain, parameter, generation): not chain 0's first sample
FRACTION_WORLD = (3, 2, 7)
# worlds whose reference misses a precondition of test_stats_reference.py at seed 0 get another seed here (never a weaker bound):
# with two split chains of two samples each R-hat is anywhere between 0.7 and 10, and five parameters have to fall into (0.9, 1.5)
# at once -- 256 is the first seed at which they do
WORLD_SEEDS = {(1, 5, 4): 256}


def mixing_matrix(d, rng):
    """Dense, well conditioned, rows of unit length: every covariance entry is different and every parameter has variance 1
    before its scaling."""
    A = np.eye(d) + 0.5 * rng.standard_normal((d, d)) / np.sqrt(d)
    return A / np.linalg.norm(A, axis=1, keepdims=True)


def scales(d, offsets=True):
    k = np.arange(d) % len(SDS)
    return (np.array(OFFSETS)[k] if offsets else np.zeros(d)), np.array(SDS)[k]


@functools.lru_cache(maxsize=None)
def _world(N, d, G, offsets, seed):
    rng = np.random.default_rng([N, d, G, seed])
    A = mixing_matrix(d, rng)
    z = rng.standard_normal((N, d, G))
    x = np.einsum("pq,nqg->npg", A, z) + CHAIN_SD * rng.standard_normal((N, d, 1))
    off, sd = scales(d, offsets)
    x = off[None, :, None] + sd[None, :, None] * x
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x


def world(N, d, G, offsets=True):
    """Read-only (N, d, G) chain history, column-major."""
    return _world(N, d, G, bool(offsets), WORLD_SEEDS.get((N, d, G), 0))


def with_dropped_sample_overwritten(chain):
    """An odd window's last generation set to 1e300: utils.jl:4-8 never reads it."""
    assert chain.shape[2] % 2 == 1
    out = np.array(chain, order="F")
    out[:, :, -1] = 1e300
    return out


def constant_in_time(N=5, d=3, G=12):
    """Chains constant in time but different from each other, at offset 1e6: W = 0 and B > 0, R-hat = +inf."""
    rng = np.random.default_rng([N, d, G, 77])
    return np.asfortranarray(np.broadcast_to(1e6 + rng.standard_normal((N, d, 1)), (N, d, G)))


def all_identical(N=5, d=3, G=12):
    """Every sample the same: W = 0 and B = 0, R-hat = nan.  (1000000.25 has 22 significant bits: the sum of any number of copies
    a test can hold is exact in every order, so the grand mean is the value itself and B is exactly 0.)"""
    return np.asfortranarray(np.full((N, d, G), 1000000.25))


def contaminated(value):
    """World CONTAMINATED with `value` in one sample of parameter POISON_AT[1]."""
    out = np.array(world(*CONTAMINATED), order="F")
    out[POISON_AT] = value
    return out


# ---- log_obj histories --------------------------------------------------------------------------------------------------------
ACCEPT_SHAPES = [(1, 2), (63, 3), (64, 34), (65, 1026), (3, 32770), (4100, 40)]


def accept_chunk_length(N, G):
    """Differences per time chunk of the accept-ratio kernel at this shape (the host's plan restated: chains in groups of 64,
    up to 1024 chunks of at least 32 differences, fewer when the groups already fill the chip).  Only the deterministic case uses
    it, to put its changes on the chunk boundaries; what the kernel must return does not depend on it."""
    cb = (N + 63) // 64
    nchunk = max(1, min((G - 1 + 31) // 32, 1024, (4096 + cb - 1) // cb))
    return (G - 1 + nchunk - 1) // nchunk


@functools.lru_cache(maxsize=None)
def _logobj_random(N, G):
    rng = np.random.default_rng([N, G, 5])
    p = np.linspace(0.0, 1.0, N) if N > 1 else np.array([0.5])        # chain c keeps its value with probability p_c
    lo = np.empty((N, G), order="F")
    lo[:, 0] = rng.standard_normal(N)
    for g in range(1, G):
        keep = rng.random(N) < p
        lo[:, g] = np.where(keep, lo[:, g - 1], rng.standard_normal(N))
    lo.setflags(write=False)
    return lo


def logobj_random(N, G):
    """Chain 0 changes every generation (ratio 1.0), chain N-1 never (ratio 0.0), the others in between."""
    return _logobj_random(N, G)


def logobj_on_chunk_boundaries(N, G, phase):
    """A change at every difference t = k * chunk length + phase (t = 1 .. G-1 is the difference between generations t-1 and t)
    and nowhere else.  phase 0: the last difference of each chunk; phase 1: the first, whose left sample belongs to the chunk
    before.  Every chain the same, so the expected count is one number."""
    per = accept_chunk_length(N, G)
    t = np.arange(G)
    steps = np.cumsum((t >= 1) & (t % per == phase % per))
    return np.asfortranarray(np.broadcast_to(steps.astype(np.float64)[None, :], (N, G)))


def logobj_uncountable(G=70):
    """Pairs that look like a change and are none, and the reverse: 0.0 / -0.0 alternating (difference +-0: not counted),
    +Inf or -Inf throughout (difference NaN: counted, utils.jl:61), and finite values that reach +Inf half way."""
    lo = np.zeros((5, G), order="F")
    lo[0, 1::2] = -0.0
    lo[1] = np.inf
    lo[2] = -np.inf
    lo[3, :G // 2] = 1.5
    lo[3, G // 2:] = np.inf
    lo[4, ::2] = -0.0
    return lo, np.array([0, G - 1, G - 1, G - G // 2, 0], dtype=np.int64)


# ---- references, computed once and shared ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rhat_reference(N, d, G, offsets=True):
    r = R.rhat_gelman(world(N, d, G, offsets))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def meancov_reference(N, d, G, offsets=True):
    m, c = R.mean_cov_chain(world(N, d, G, offsets))
    m.setflags(write=False)
    c.setflags(write=False)
    return m, c


def rhat_chunk_lengths(G):
    """Lengths of the time chunks of one half in the R-hat moments kernel (the host's plan restated: one chunk per 32 samples of
    the half, 32 at the most, the last one takes what is left).  Used only to show that the shapes reach the edges they are for."""
    n = G // 2
    nchunk = min(max(1, n // 32), 32)
    per = (n + nchunk - 1) // nchunk
    return [max(0, min(per, n - k * per)) for k in range(nchunk)]


def meancov_chunk_lengths(N, d, G):
    """The same for the mean / covariance kernel: up to 512 chunks of at least 16 generations, fewer when chains x tile pairs
    already fill the chip."""
    T = (d + 7) // 8
    groups = ((N + 255) // 256) * (T * (T + 1) // 2)
    nchunk = max(1, min((G + 15) // 16, 512, (2048 + groups - 1) // groups))
    per = (G + nchunk - 1) // nchunk
    return [max(0, min(per, G - k * per)) for k in range(nchunk)]


def all_worlds():
    """Every non-degenerate world of the lists above, once."""
    seen, out = set(), []
    for w in MEANCOV_WORLDS + RHAT_WORLDS + [CONTAMINATED]:
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def has_rhat(w):
    return w[2] >= 4
