"""Inputs shared by test_ess_reference.py (no GPU: the reference against exact arithmetic, the preconditions and the headroom of
the tolerances, the host finisher) and test_gpu_ess.py (the device): chain histories that are AR(1) in time -- the worlds of
stats_cases.py are white noise, their autocovariance beyond lag 0 is sampling noise and would exercise nothing -- at the smallest
shapes that reach each edge of the autocovariance kernel, and their references, computed once (ess_reference.py)."""
import functools

import numpy as np

import ess_reference as E
import stats_cases as S

PHI = (0.0, 0.5, 0.9, -0.5, 0.98, 0.7)          # by p % 6: white, mixing, slow, antithetic, very slow, in between
CHAIN_SD = 0.05

TL = 32                                         # lags per tile of the kernel (ACF_TL)
WORLDS = [
    (257, 6, 131),     # one lane past four waves; odd window; L = 64: two full tiles and one lag
    (64, 3, 260),      # L = 129: the tile count is not a power of two
    (3, 6, 2051),      # long series, few chains, L = 1024, many empty lanes; pairs up to 82
    (1, 2, 40),        # one chain
    (65, 7, 20),       # L = 9, less than one tile; a negative tau
    (600, 2, 64),      # chains past one workgroup of the reduction, one chunk
    (63, 12, 66),      # one lane short of a wave per parameter
    (2, 1, 5),         # L = 1
    (1, 1, 4),         # L = 1, zero pairs summed, ESS at the cap
    # the chunk plan below at N d = 4: n = 191, 192, 193 put the end of the half one sample before, at and one sample after a
    # chunk boundary (chunks of 96, 64, 96 samples)
    (2, 2, 382), (2, 2, 384), (2, 2, 387),
]
FRACTION_WORLD = (3, 2, 9)
# worlds whose reference misses the margin precondition of test_ess_reference.py at seed 0 get another seed here (never a
# weaker bound)
WORLD_SEEDS = {}


def chunk_lengths(N, d, G):
    """Left samples per time chunk of one half in acf_products_kernel (the host's plan, acf_chunks, restated): chunks are whole
    numbers of tiles long, at least two tiles, at most 64 of them, and no more than it takes for 2 halves x 4 tiles x chunks x
    waves to reach 4096 waves.  Used only to show that the shapes reach the edges they are for."""
    n = G // 2
    waves = (N * d + 63) // 64
    want = (4096 + 8 * waves - 1) // (8 * waves)
    k = max(1, min(n // (2 * TL), want, 64))
    per = (((n + k - 1) // k) + TL - 1) // TL * TL
    nchunk = (n + per - 1) // per
    return [min(per, n - c * per) for c in range(nchunk)]


@functools.lru_cache(maxsize=None)
def _world(N, d, G, seed):
    rng = np.random.default_rng([N, d, G, seed, 11])
    e = rng.standard_normal((N, d, G))
    phi = np.array(PHI)[np.arange(d) % len(PHI)][None, :]
    x = np.empty((N, d, G))
    x[..., 0] = e[..., 0]
    for g in range(1, G):
        x[..., g] = phi * x[..., g - 1] + np.sqrt(1 - phi ** 2) * e[..., g]
    x = x + CHAIN_SD * rng.standard_normal((N, d, 1))
    off, sd = S.scales(d)
    x = np.asfortranarray(off[None, :, None] + sd[None, :, None] * x)
    x.setflags(write=False)
    return x


def world(N, d, G):
    """Read-only (N, d, G) chain history, column-major."""
    return _world(N, d, G, WORLD_SEEDS.get((N, d, G), 0))


@functools.lru_cache(maxsize=None)
def reference(N, d, G, max_lag=0):
    return E.ess(world(N, d, G), max_lag)


def poisoned(value, w=(257, 6, 131), at=(100, 4, 17)):
    """World `w` with `value` in one sample (chain, parameter, generation): not chain 0's first."""
    out = np.array(world(*w), order="F")
    out[at] = value
    return out, at[1]


ids = lambda w: "x".join(str(v) for v in w)      # noqa: E731
