"""Inputs and the references shared by test_density_reference.py (no GPU: the references against NumPy's own histograms, the host
half of the library, and the preconditions that give the GPU cases their meaning) and test_gpu_density.py (the kernels behind
demcz_histogram, demcz_histogram2d and demcz_hdi and their Python faces).  NumPy only.

The bin rule: edges = np.linspace(lo, hi, nbins + 1); x lies in bin k iff edges[k] <= x < edges[k+1], the
last bin also takes x == edges[nbins]; x < edges[0] is below, x > edges[nbins] above, a NaN is counted apart.  The reference
places a draw with np.searchsorted on the table.  The HDI: the sorted-array formula with the device's tie and NaN rules."""
import functools
from collections import namedtuple

import numpy as np

import quantile_cases as Q
import stats_cases as S

Hist = namedtuple("Hist", "counts edges below above nan")
Hist2 = namedtuple("Hist2", "counts outside")

# (N, d, G): chain blocks that are not full (N = 1, 63, 65, 257), d = 1, 2, 9, 20, 33, one generation, and at N = 3 a window long
# enough for several time chunks per workgroup
WORLDS = [(1, 1, 1), (63, 2, 5), (65, 9, 7), (257, 20, 3), (5, 33, 4), (3, 2, 2051), (64, 1, 1)]
NBINS = (1, 2, 33, 256, 4096)
GRIDS = ((1, 1), (32, 17), (128, 128))
SPREAD_WORLD = (257, 20, 3)                       # 33 automatic bins: the 64 lanes of a wave fall into many of them
HDI_PROBS = (0.5, 0.94, 0.2, 0.999, 0.001)
ALL36 = [(p, q) for p in range(9) for q in range(p + 1, 9)]
MIXED_PAIRS = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (3, 1), (1, 3), (0, 1)]      # 1 in both positions, (q, p) next to (p, q), a repeat


def ids(w):
    return "x".join(str(v) for v in w)


def draws(chain, p):
    return np.ascontiguousarray(np.asarray(chain)[:, p, :]).ravel()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the bin rule ------------------------------------------------------------------------------------------------------------------
def edges_of(lo, hi, nb):
    return np.linspace(lo, hi, nb + 1)


def auto_range(chain):
    """d x 2: the smallest and largest draw of every parameter; (x - 0.5, x + 0.5) where they are equal."""
    chain = np.asarray(chain)
    lo, hi = chain.min(axis=(0, 2)), chain.max(axis=(0, 2))
    same = lo == hi
    return np.stack([np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)], axis=1)


def full_range(rng, chain):
    d = np.asarray(chain).shape[1]
    if rng is None:
        return auto_range(chain)
    r = np.asarray(rng, dtype=np.float64)
    return np.broadcast_to(r, (d, 2)) if r.shape == (2,) else r


def place(x, e):
    """The bin of every draw: 0..nb-1, or -1 (below), -2 (above), -3 (NaN)."""
    nb = e.size - 1
    k = np.searchsorted(e, x, side="right") - 1
    k = np.where(x == e[nb], nb - 1, k)
    k = np.where(x < e[0], -1, k)
    k = np.where(x > e[nb], -2, k)
    return np.where(np.isnan(x), -3, k)


def hist_reference(chain, nb, rng=None):
    chain = np.asarray(chain)
    d = chain.shape[1]
    r = full_range(rng, chain)
    out = Hist(np.zeros((d, nb), dtype=np.int64), np.empty((d, nb + 1)), *(np.zeros(d, dtype=np.int64) for _ in range(3)))
    for p in range(d):
        e = out.edges[p] = edges_of(r[p, 0], r[p, 1], nb)
        k = place(draws(chain, p), e)
        out.counts[p] = np.bincount(k[k >= 0], minlength=nb)
        out.below[p], out.above[p], out.nan[p] = (k == -1).sum(), (k == -2).sum(), (k == -3).sum()
    return out


def hist2d_reference(chain, pairs, nbx, nby, rng=None):
    chain = np.asarray(chain)
    r = full_range(rng, chain)
    counts = np.zeros((len(pairs), nbx, nby), dtype=np.int64)
    outside = np.zeros(len(pairs), dtype=np.int64)
    for i, (p, q) in enumerate(pairs):
        kx = place(draws(chain, p), edges_of(r[p, 0], r[p, 1], nbx))
        ky = place(draws(chain, q), edges_of(r[q, 0], r[q, 1], nby))
        inside = (kx >= 0) & (ky >= 0)
        np.add.at(counts[i], (kx[inside], ky[inside]), 1)
        outside[i] = (~inside).sum()
    return Hist2(counts, outside)


def same_hist(got, ref):
    return (np.array_equal(got.counts, ref.counts) and np.array_equal(bits(got.edges), bits(ref.edges))
            and np.array_equal(got.below, ref.below) and np.array_equal(got.above, ref.above) and np.array_equal(got.nan, ref.nan))


# ---- the highest-density interval ----------------------------------------------------------------------------------------------------
def hdi_steps(S_, prob):
    return min(int(np.floor(float(prob) * float(S_))), S_ - 1)


def hdi_widths(x, prob):
    """(sorted draws with -0.0 taken as 0.0, m, the widths s[i + m] - s[i] for 0 <= i < S - m)."""
    s = np.sort(np.asarray(x, dtype=np.float64) + 0.0)
    m = hdi_steps(s.size, prob)
    with np.errstate(all="ignore"):
        return s, m, s[m:] - s[:s.size - m]


def hdi_reference(chain, probs):
    """d x nprob x 2: ties to the smallest i, a NaN width is no candidate, no candidate or a NaN draw gives NaN, NaN."""
    chain = np.asarray(chain)
    d = chain.shape[1]
    out = np.full((d, len(probs), 2), np.nan)
    for p in range(d):
        x = draws(chain, p)
        if np.isnan(x).any():
            continue
        for j, prob in enumerate(probs):
            s, m, wd = hdi_widths(x, prob)
            cand = ~np.isnan(wd)
            if cand.any():
                i = int(np.flatnonzero(cand & (wd == wd[cand].min()))[0])
                out[p, j] = s[i], s[i + m]
    return out


def hdi_plain(x, prob):
    """The plain formula on a tie-free sample without special values."""
    s = np.sort(x)
    m = int(np.floor(prob * s.size))
    i = int(np.argmin(s[m:] - s[:s.size - m]))
    return s[i], s[i + m]


def multimodal_reference(counts, edges, prob):
    """Per parameter the list of (lo, hi): bins by falling count, among equals by rising index, until their share reaches prob."""
    out = []
    for c, e in zip(counts, edges):
        total = int(c.sum())
        order = sorted(range(c.size), key=lambda k: (-int(c[k]), k))
        taken, have = [], 0
        for k in order:
            if total == 0 or have >= prob * total:
                break
            taken.append(k)
            have += int(c[k])
        taken.sort()
        runs = []
        for k in taken:
            if runs and runs[-1][1] == k - 1:
                runs[-1][1] = k
            else:
                runs.append([k, k])
        out.append([(float(e[a]), float(e[b + 1])) for a, b in runs])
    return out


# ---- worlds beyond stats_cases -------------------------------------------------------------------------------------------------------
def _nan(negative):
    return np.array([0xFFF8000000000000 if negative else 0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


@functools.lru_cache(maxsize=None)
def edge_world(nb):
    """((65, 2, G) chain, its 2 x 2 range): every edge of the two tables, the doubles one ulp below and one ulp above each, and
    -0.0 (parameter 0's first edge is 0.0), padded with draws inside the range."""
    rng = np.array([[0.0, 3.3], [-0.7, 0.1]])
    cols = []
    for lo, hi in rng:
        e = edges_of(lo, hi, nb)
        cols.append(np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [-0.0, 0.0]]))
    G = -(-cols[0].size // 65)
    gen = np.random.default_rng([nb, 14])
    x = np.empty((65, 2, G), order="F")
    for p, (lo, hi) in enumerate(rng):
        v = np.concatenate([cols[p], gen.uniform(lo, hi, 65 * G - cols[p].size)])
        x[:, p, :] = gen.permutation(v).reshape(G, 65).T
    x.setflags(write=False)
    rng.setflags(write=False)
    return x, rng


@functools.lru_cache(maxsize=None)
def out_of_range_world():
    """((65, 3, 9) chain, its 3 x 2 range): quantile_cases.specials() (+-0.0, +-inf, subnormals, runs of duplicates) with a NaN of
    either sign in every parameter, under a range from the 15 % to the 85 % point of each parameter's finite draws."""
    x = np.array(Q.specials(), order="F")
    for p in range(3):
        x[7 + p, p, 2], x[40 + p, p, 6] = _nan(False), _nan(True)
    rng = np.empty((3, 2))
    for p in range(3):
        v = np.sort(draws(x, p)[np.isfinite(draws(x, p))])
        rng[p] = v[int(0.15 * v.size)], v[int(0.85 * v.size)]
    x.setflags(write=False)
    rng.setflags(write=False)
    return x, rng


@functools.lru_cache(maxsize=None)
def piled_world():
    """((128, 2, 40) chain, its range): parameter 0 is a unit normal under the range (-100, 100): at 33 bins the central one holds
    nearly every draw, so whole runs of a wave's generations hit one bin; parameter 1 spreads over its range."""
    gen = np.random.default_rng(15)
    x = np.asfortranarray(np.stack([gen.standard_normal((128, 40)), gen.uniform(-5.0, 5.0, (128, 40))], axis=1))
    rng = np.array([[-100.0, 100.0], [-5.0, 5.0]])
    x.setflags(write=False)
    rng.setflags(write=False)
    return x, rng


@functools.lru_cache(maxsize=None)
def constant_world():
    """(65, 3, 4): parameter 1 is one value throughout (the automatic range is x -+ 0.5), parameter 2 sits at offset -3e5."""
    x = np.array(S.world(65, 3, 4), order="F")
    x[:, 1, :] = 1000000.25
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def hdi_special_world():
    """(65, 3, 9): specials() -- parameter 0 holds +-inf, so some widths are inf - inf; parameter 1 holds 135 equal draws of
    chains that stood still, so the smallest width, 0, is attained at many starts."""
    return Q.specials()


def wave_bins(chain, p, e):
    """Per (block of 64 chains, generation): the number of distinct bins among the lanes of that wave's load."""
    chain = np.asarray(chain)
    N, _, G = chain.shape
    out = np.zeros(((N + 63) // 64, G), dtype=np.int64)
    for b in range(out.shape[0]):
        for g in range(G):
            out[b, g] = np.unique(place(chain[64 * b:64 * b + 64, p, g], e)).size
    return out
