"""``HipEngine``: one ``demcz_handle`` (one GPU, one shard of chains) behind a small Python face.

The drivers in ``sampler.py`` talk to an engine through the methods below and nothing else;
the product only ever constructs ``HipEngine``.  (tests/ inject an oracle-backed engine with
the same methods to exercise the host logic, e.g. the world_size-2 gloo tests, on machines
without a GPU.)
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import DemczError
from .targets import is_device_target

# per parameter: effective sample size, autocorrelation time (uncapped), var+ (R-hat's varhat), pairs summed by Geyer's
# initial monotone sequence, and whether a non-positive pair ended it (0: the lags ran out, ess is an upper bound)
ESS = namedtuple("ESS", "ess tau varplus pairs converged")


def ess_from_sums(m, n, sums, between):
    """demcz_ess_from_sums (host code, no device): `sums` is d x nlags from lag 0, sum over all m split chains of n c_j(t);
    `between` is sum_j (mean_j - grand)^2 per parameter."""
    sums = _lib.f64(sums, "F")
    d, nlags = sums.shape
    between = _lib.f64(between)
    if between.shape != (d,):
        raise ValueError("between must have d entries")
    out = ESS(np.empty(d), np.empty(d), np.empty(d), np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int32))
    rc = _lib.load().demcz_ess_from_sums(d, int(m), int(n), nlags, _lib.ptr(sums), _lib.ptr(between), _lib.ptr(out.ess), _lib.ptr(out.tau),
                                         _lib.ptr(out.varplus), _lib.ptr(out.pairs, _lib._lp), _lib.ptr(out.converged, _lib._ip))
    if rc != 0:
        raise DemczError(rc, "demcz_ess_from_sums: d >= 1, n >= 2, nlags >= 1")
    return out


# quantiles per parameter (d x nq) and, on request, the two order statistics they were formed from (lower = x_(lo), upper = x_(hi))
Quantiles = namedtuple("Quantiles", "q lower upper")
# the best draw of a window: max of log_obj, 0-based chain, generation, chain[chain, :, generation]
Best = namedtuple("Best", "bestval chain generation bestpar")
# per parameter: rank-normalised split R-hat (the larger of bulk and folded), bulk-ESS and tail-ESS (Vehtari et al. 2021)
RankDiagnostics = namedtuple("RankDiagnostics", "rhat_rank ess_bulk ess_tail")


class Crossover(namedtuple("Crossover", "ncr delta_max weights tried accepted")):
    """HipEngine.crossover: the setting and, per CR class, the crossover steps tried and accepted over the handle's life."""
    __slots__ = ()

    @property
    def accept_rate(self):
        """accepted / tried per class (NaN where a class was never tried)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.accepted / self.tried.astype(np.float64)


class CrossoverAdapt(namedtuple("CrossoverAdapt", "every until min_weight weights dist tried rsd updates")):
    """HipEngine.crossover_adapt: the setting of the adaptation of the CR class weights and its state on the device -- per class
    the weights, the quantised squared jump distance (units of 1/65536) and the steps tried since adaptation started; the
    reciprocal standard deviation of every parameter over the chains at the last update; the updates made."""
    __slots__ = ()

    @property
    def jump_per_try(self):
        """normalised squared jump distance per step tried, per class (NaN where a class was never tried): what the weights follow"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.dist / 65536.0 / self.tried.astype(np.float64)

    @property
    def shares(self):
        """weights / W: the probability of each class"""
        return self.weights / float(self.weights.sum())



class PPC(namedtuple("PPC", "gt eq nan total names")):
    """A posterior predictive check (demcz_ppc): per column of the program, how many of the ``total`` draws had a value greater
    than the observed one (``gt``), equal to it (``eq``), or NaN (``nan``) -- int64 arrays of m entries; integer counts, so the
    records of shards add field by field (``+``)."""
    __slots__ = ()

    @property
    def p_value(self):
        """P(T_rep >= T_obs) over the draws whose value is a number: (gt + eq) / (total - nan)."""
        with np.errstate(all="ignore"):
            return (self.gt + self.eq) / (self.total - self.nan)

    @property
    def mid_p(self):
        """The mid p-value, which counts a tie as half: (gt + eq / 2) / (total - nan)."""
        with np.errstate(all="ignore"):
            return (self.gt + self.eq / 2) / (self.total - self.nan)

    def __add__(self, other):
        return PPC(self.gt + other.gt, self.eq + other.eq, self.nan + other.nan, self.total + other.total, self.names)


def _ppc_observed(observed, m):
    if observed is None:
        return None
    obs = _lib.f64(np.ravel(observed))
    if obs.shape != (m,):
        raise ValueError("observed must have m entries")
    return obs


def ppc_record(counts, total, names=None):
    """The ``PPC`` of demcz_ppc's 3 m counts (gt, eq, nan of column 0, then of column 1, ...)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    return PPC(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), int(total), names)


class Histogram(namedtuple("Histogram", "counts edges below above nan")):
    """Marginal histograms (demcz_histogram): counts d x nbins int64, edges d x (nbins + 1), and per parameter the draws below the
    range, above it, and NaN.  Bin k holds edges[k] <= x < edges[k+1]; the last bin also holds x == edges[nbins]."""
    __slots__ = ()

    @property
    def density(self):
        """counts / (in-range total * bin width): integrates to one over the range (NaN for a parameter with no draw in range)."""
        with np.errstate(all="ignore"):
            return self.counts / (self.counts.sum(axis=1, keepdims=True) * np.diff(self.edges, axis=1))

    def mode(self):
        """The centre of the fullest bin of every parameter, the lowest on ties."""
        k = np.argmax(self.counts, axis=1)
        p = np.arange(self.counts.shape[0])
        return 0.5 * (self.edges[p, k] + self.edges[p, k + 1])

    def hdi(self, prob):
        """The multimodal highest-density region from the bins (host code): bins are taken in order of falling count, among
        equals in order of rising index, until their share of the in-range draws reaches ``prob``; the result is the union of
        adjacent taken bins: per parameter a list of (lo, hi) intervals (empty with no draw in range)."""
        prob = float(prob)
        if not 0.0 < prob < 1.0:
            raise ValueError("prob must lie inside (0, 1)")
        out = []
        for c, e in zip(self.counts, self.edges):
            total = int(c.sum())
            if total == 0:
                out.append([])
                continue
            order = np.argsort(-c, kind="stable")
            ntake = int(np.searchsorted(np.cumsum(c[order]), prob * total, side="left")) + 1
            taken = np.sort(order[:min(ntake, c.size)])
            cuts = np.flatnonzero(np.diff(taken) > 1)
            first = np.concatenate([[0], cuts + 1])
            last = np.concatenate([cuts, [taken.size - 1]])
            out.append([(float(e[taken[a]]), float(e[taken[b] + 1])) for a, b in zip(first, last)])
        return out


# pairwise histograms (demcz_histogram2d): counts npairs x nbx x nby int64, pairs npairs x 2, edges = (edges_x d x (nbx + 1),
# edges_y d x (nby + 1)): pair (p, q) is binned by edges_x[p] and edges_y[q]; outside: draws with a coordinate out of range or NaN
Histogram2D = namedtuple("Histogram2D", "counts pairs edges outside")


def histogram_edges(nbins, lo, hi):
    """demcz_histogram_edges (host code, no device): the table np.linspace(lo, hi, nbins + 1) of one parameter, as the library
    forms it."""
    out = np.empty(int(nbins) + 1 if nbins >= 1 else 1)
    rc = _lib.load().demcz_histogram_edges(int(nbins), float(lo), float(hi), _lib.ptr(out))
    if rc != 0:
        raise DemczError(rc, "demcz_histogram_edges: 1 <= nbins <= 4096 and lo < hi, both finite, hi - lo finite")
    return out


def hdi_steps(S, probs):
    """demcz_hdi_steps (host code, no device): min(floor(prob S), S - 1) per probability."""
    probs = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    out = np.zeros(probs.size, dtype=np.int64)
    rc = _lib.load().demcz_hdi_steps(int(S), probs.size, _lib.ptr(probs), _lib.ptr(out, _lib._lp))
    if rc != 0:
        raise DemczError(rc, "demcz_hdi_steps: S >= 1 and 1 to 16 probabilities inside (0, 1)")
    return out


def _range_args(rng, d):
    """(lo, hi) as two contiguous d-vectors, or (None, None): ``rng`` is None, one (lo, hi) for every parameter, or d x 2."""
    if rng is None:
        return None, None
    r = np.asarray(rng, dtype=np.float64)
    if r.shape == (2,):
        r = np.broadcast_to(r, (d, 2))
    if r.shape != (d, 2):
        raise ValueError("range must be (lo, hi) or d x 2")
    return np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])


def _pairs_arg(pairs, d):
    if pairs is None:
        pairs = [(p, q) for p in range(d) for q in range(p + 1, d)]
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    if pr.shape[0] < 1:
        raise ValueError("at least one pair (d >= 2)")
    return pr


def _bins2(bins):
    nbx, nby = (bins, bins) if np.ndim(bins) == 0 else bins
    return int(nbx), int(nby)


# PSIS-LOO and WAIC (demcz_loo, demcz_loo_columns).  Per observation: elpd_loo_i, pareto_k, n_tail, lppd_i, p_waic_i,
# p_loo_i = lppd_i - elpd_loo_i and elpd_waic_i = lppd_i - p_waic_i; the totals elpd_loo, p_loo, elpd_waic, p_waic; se_elpd_loo and
# se_elpd_waic = sqrt(nobs var(pointwise, divisor nobs - 1)); k_threshold = min(1 - 1 / log10(S), 0.7) of the S draws; bad_k: the
# observations with pareto_k above it; names
LOO = namedtuple("LOO", "elpd_loo_i pareto_k n_tail lppd_i p_waic_i p_loo_i elpd_waic_i elpd_loo p_loo elpd_waic p_waic se_elpd_loo "
                        "se_elpd_waic k_threshold bad_k names")


def _pointwise_se(v):
    """sqrt(nobs * var(v, divisor nobs - 1)); NaN for one observation."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.sqrt(v.size * np.var(v, ddof=1))) if v.size > 1 else float("nan")


def loo_record(elpd_loo_i, pareto_k, n_tail, lppd_i, p_waic_i, S, names=None):
    """The ``LOO`` record of the five per-observation outputs of demcz_loo / demcz_loo_columns over S draws (host code)."""
    elpd_loo_i, pareto_k, lppd_i, p_waic_i = (np.asarray(a, dtype=np.float64) for a in (elpd_loo_i, pareto_k, lppd_i, p_waic_i))
    with np.errstate(all="ignore"):
        p_loo_i = lppd_i - elpd_loo_i
        elpd_waic_i = lppd_i - p_waic_i
        thr = min(1.0 - 1.0 / np.log10(float(S)), 0.7) if S > 1 else float("-inf")
    return LOO(elpd_loo_i, pareto_k, np.asarray(n_tail, dtype=np.int64), lppd_i, p_waic_i, p_loo_i, elpd_waic_i,
               float(elpd_loo_i.sum()), float(p_loo_i.sum()), float(elpd_waic_i.sum()), float(p_waic_i.sum()),
               _pointwise_se(elpd_loo_i), _pointwise_se(elpd_waic_i), float(thr), np.flatnonzero(pareto_k > thr),
               list(names) if names is not None else None)


def loo_compare(a, b):
    """(elpd_diff, se_diff) of two ``LOO`` records of the same observations, a minus b: the sum of the paired differences of
    elpd_loo_i and sqrt(nobs * var(differences, divisor nobs - 1)).  Host code."""
    if a.elpd_loo_i.shape != b.elpd_loo_i.shape:
        raise ValueError("the two records must cover the same observations")
    diff = a.elpd_loo_i - b.elpd_loo_i
    return float(diff.sum()), _pointwise_se(diff)


def psis_tail_length(S, r_eff=1.0):
    """demcz_psis_tail_length (host code, no device): M = ceil(min(S / 5, 3 sqrt(S / r_eff)))."""
    M = C.c_int64()
    rc = _lib.load().demcz_psis_tail_length(int(S), float(r_eff), C.byref(M))
    if rc != 0:
        raise DemczError(rc, "demcz_psis_tail_length: S >= 1 and r_eff in (0, inf)")
    return M.value


def gpd_fit(x_ascending):
    """demcz_gpd_fit (host code, no device): (k, sigma, khat) of n >= 5 exceedances in ascending order."""
    x = np.ascontiguousarray(x_ascending, dtype=np.float64)
    k, sigma, khat = C.c_double(), C.c_double(), C.c_double()
    rc = _lib.load().demcz_gpd_fit(x.size, _lib.ptr(x), C.byref(k), C.byref(sigma), C.byref(khat))
    if rc != 0:
        raise DemczError(rc, "demcz_gpd_fit: at least 5 exceedances")
    return k.value, sigma.value, khat.value


def _loo_outputs(n):
    return np.empty(n), np.empty(n), np.zeros(n, dtype=np.int64), np.empty(n), np.empty(n)


def _r_eff_arg(r_eff, n):
    if r_eff is None:
        return None
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(r_eff, dtype=np.float64), (n,)))
    return r


# The marginal likelihood by bridge sampling (demcz_bridge).  logml and its standard error se_logml; iterations and converged of the
# fixed-point iteration; n_post and n_prop, the draws on either side; neff as used; n_nan, the proposal draws whose log-density was
# NaN (taken as -inf); ess_f2; mean and L of the proposal N(mean, L L^T)
Bridge = namedtuple("Bridge", "logml se_logml iterations converged n_post n_prop neff n_nan ess_f2 mean L")
# demcz_bridge_iterate: moments = (mean f1, var f1, mean f2, var f2) at the final rho; f2: a DerivedHistory, or None
BridgeIteration = namedtuple("BridgeIteration", "logml iterations converged moments n_nan f2")

BRIDGE_SEED_XOR = 0x9E3779B97F4A7C15     # the default seed of the proposal's streams is the run's seed XOR this constant


def bridge_seed(run_seed):
    """The documented default seed of ``HipEngine.bridge``: the run's seed XOR ``BRIDGE_SEED_XOR`` (the 64-bit golden ratio), so
    that the proposal does not replay the sampler's Philox streams."""
    return (int(run_seed) ^ BRIDGE_SEED_XOR) & (2**64 - 1)


def bridge_se(moments, n_prop, ess_f2):
    """se_logml = sqrt(var f1 / (N2 mean f1^2) + var f2 / (ESS(f2) mean f2^2)) as demcz_bridge forms it (host code)."""
    m1, v1, m2, v2 = (float(v) for v in moments)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v1) / (np.float64(n_prop) * (np.float64(m1) * m1))
                             + np.float64(v2) / (np.float64(ess_f2) * (np.float64(m2) * m2))))


def _bridge_outputs(d):
    return dict(logml=C.c_double(), se=C.c_double(), it=C.c_int64(), conv=C.c_int32(), n1=C.c_int64(), n2=C.c_int64(),
                neff=C.c_double(), nnan=C.c_int64(), ess=C.c_double(), mean=np.empty(d), L=np.empty((d, d), order="F"))


def _bridge_out_args(o):
    return [C.byref(o["logml"]), C.byref(o["se"]), C.byref(o["it"]), C.byref(o["conv"]), C.byref(o["n1"]), C.byref(o["n2"]),
            C.byref(o["neff"]), C.byref(o["nnan"]), C.byref(o["ess"]), _lib.ptr(o["mean"]), _lib.ptr(o["L"])]


def _bridge_record(o):
    return Bridge(o["logml"].value, o["se"].value, o["it"].value, bool(o["conv"].value), o["n1"].value, o["n2"].value,
                  o["neff"].value, o["nnan"].value, o["ess"].value, o["mean"], o["L"])


def _bridge_ml(mean, L, d):
    mean = _lib.f64(mean)
    L = _lib.f64(L, "F")
    if mean.shape != (d,) or L.shape != (d, d):
        raise ValueError("mean must have d entries and L must be d x d")
    return mean, L


def bridge_iterate(post, prop, g_from=None, g_to=None, gp_from=None, gp_to=None, neff=None, tol=1e-10, max_iter=1000, want_f2=False):
    """The fixed-point iteration of bridge sampling on two one-column ``DerivedHistory`` objects on one device
    (demcz_bridge_iterate): ``post`` holds a1 = log_obj - log g at the posterior draws, ``prop`` a2 = logobj - log g at the
    proposal's; the windows default to all of either.  ``neff``: the effective number of posterior draws (None: all of them).
    Returns a ``BridgeIteration``; with ``want_f2`` its ``f2`` is a ``DerivedHistory`` (a context manager) whose ``ess`` gives
    the error estimate's ESS(f2), see ``bridge_se``."""
    g_from = post.g_from if g_from is None else int(g_from)
    g_to = post.g_to if g_to is None else int(g_to)
    gp_from = prop.g_from if gp_from is None else int(gp_from)
    gp_to = prop.g_to if gp_to is None else int(gp_to)
    logml, it, conv, nnan = C.c_double(), C.c_int64(), C.c_int32(), C.c_int64()
    mom = np.empty(4)
    f2 = C.c_void_p()
    post._chk(post._L.demcz_bridge_iterate(post._h, g_from, g_to, prop._h, gp_from, gp_to, 0.0 if neff is None else float(neff),
                                           float(tol), int(max_iter), C.byref(logml), C.byref(it), C.byref(conv), _lib.ptr(mom),
                                           C.byref(nnan), C.byref(f2) if want_f2 else None))
    hist = DerivedHistory(post._L, f2, post.N, 1, g_from, g_to, ["f2"]) if want_f2 else None
    return BridgeIteration(logml.value, it.value, bool(conv.value), mom, nnan.value, hist)


def bayes_factor(a, b):
    """(log_bf, se) of two ``Bridge`` records, a over b: logml_a - logml_b and sqrt(se_a^2 + se_b^2).  Host code."""
    with np.errstate(all="ignore"):
        return float(a.logml - b.logml), float(np.sqrt(np.float64(a.se_logml) ** 2 + np.float64(b.se_logml) ** 2))


def post_prob(*bridges, prior=None):
    """Posterior model probabilities of ``Bridge`` records (or plain logml values): the softmax of logml + log prior on the host.
    ``prior``: one positive weight per model (default: equal); it need not sum to one."""
    lm = np.array([getattr(b, "logml", b) for b in bridges], dtype=np.float64)
    if lm.size == 0:
        raise ValueError("at least one model")
    pr = np.ones(lm.size) if prior is None else np.asarray(prior, dtype=np.float64)
    if pr.shape != lm.shape or not np.all(pr > 0):
        raise ValueError("prior must hold one positive weight per model")
    v = lm + np.log(pr)
    if np.any(np.isnan(v)):
        return np.full(lm.size, np.nan)
    e = np.exp(v - v.max())
    return e / e.sum()


def rank_to_z(r, S):
    """demcz_rank_to_z (host code, no device): the normal scores of average ranks r (1 <= r <= S) among S draws, by the operation
    sequence the device runs (Blom's offsets, Wichura's AS 241)."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    z = np.empty(r.shape)
    rc = _lib.load().demcz_rank_to_z(r.size, _lib.ptr(r), int(S), _lib.ptr(z))
    if rc != 0:
        raise DemczError(rc, "demcz_rank_to_z: 1 <= S < 2^50 and every rank in [1, S]")
    return z


def quantile_plan(S, probs):
    """demcz_quantile_plan (host code, no device): (rank_lo, rank_hi, frac) of Hyndman-Fan type 7 for S draws."""
    probs = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    nq = probs.size
    lo, hi, frac = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64), np.zeros(nq)
    rc = _lib.load().demcz_quantile_plan(int(S), nq, _lib.ptr(probs), _lib.ptr(lo, _lib._lp), _lib.ptr(hi, _lib._lp), _lib.ptr(frac))
    if rc != 0:
        raise DemczError(rc, "demcz_quantile_plan: S >= 1, 1 to 16 probabilities, each in [0, 1]")
    return lo, hi, frac


def select_step(counts, prefix, rank):
    """demcz_select_step (host code, no device): counts (d, nr, 256) int64 already added over shards, prefix (d, nr) uint64 and
    rank (d, nr) int64; returns the new (prefix, rank)."""
    prefix = np.array(prefix, dtype=np.uint64, order="F", ndmin=2)
    rank = np.array(rank, dtype=np.int64, order="F", ndmin=2)
    d, nr = prefix.shape
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.shape != (d, nr, 256) or rank.shape != (d, nr):
        raise ValueError("counts must be (d, nr, 256), prefix and rank (d, nr)")
    rc = _lib.load().demcz_select_step(d, nr, _lib.ptr(counts, _lib._lp), _lib.ptr(prefix, _lib._up), _lib.ptr(rank, _lib._lp))
    if rc != 0:
        raise DemczError(rc, "demcz_select_step: a rank is not below the total of its counts")
    return prefix, rank


def quantile_finish(key_lo, key_hi, frac, nan_count=None):
    """demcz_quantile_finish (host code, no device): keys (d, nq) uint64 -> Quantiles."""
    key_lo = np.array(key_lo, dtype=np.uint64, order="F", ndmin=2)
    key_hi = np.array(key_hi, dtype=np.uint64, order="F", ndmin=2)
    d, nq = key_lo.shape
    frac = np.ascontiguousarray(frac, dtype=np.float64)
    nan_count = None if nan_count is None else np.ascontiguousarray(nan_count, dtype=np.int64)
    if key_hi.shape != (d, nq) or frac.shape != (nq,) or (nan_count is not None and nan_count.shape != (d,)):
        raise ValueError("key_lo and key_hi must be (d, nq), frac (nq,), nan_count (d,)")
    out = Quantiles(np.empty((d, nq), order="F"), np.empty((d, nq), order="F"), np.empty((d, nq), order="F"))
    rc = _lib.load().demcz_quantile_finish(d, nq, _lib.ptr(key_lo, _lib._up), _lib.ptr(key_hi, _lib._up), _lib.ptr(frac),
                                           _lib.ptr(nan_count, _lib._lp), _lib.ptr(out.q), _lib.ptr(out.lower), _lib.ptr(out.upper))
    if rc != 0:
        raise DemczError(rc, "demcz_quantile_finish: 1 to 16 probabilities")
    return out


def select_quantiles(count_pass, S, d, probs):
    """The radix select driven from the host, for counts that have to be added over shards first: `count_pass(shift, prefix)`
    returns ((d, nprefix, 256) int64 counts, (d,) NaN counts) over ALL shards for a (d, nprefix) uint64 prefix array.  Eight
    passes; the ranks of one parameter that share a prefix share one column of the pass (demcz_quantiles does the same)."""
    lo, hi, frac = quantile_plan(S, probs)
    nq = lo.size
    rank = np.asfortranarray(np.broadcast_to(np.stack([lo, hi], axis=1).reshape(1, 2 * nq), (d, 2 * nq)))
    prefix = np.zeros((d, 2 * nq), dtype=np.uint64, order="F")
    nan = np.zeros(d, dtype=np.int64)
    for shift in range(56, -8, -8):
        uniq = [list(dict.fromkeys(prefix[p].tolist())) for p in range(d)]
        npre = max(len(u) for u in uniq)
        pre = np.full((d, npre), ~np.uint64(0), dtype=np.uint64, order="F")
        for p, u in enumerate(uniq):
            pre[p, :len(u)] = u
        counts, nan = count_pass(shift, pre)
        slot = np.array([[uniq[p].index(v) for v in prefix[p].tolist()] for p in range(d)])
        prefix, rank = select_step(np.take_along_axis(counts, slot[:, :, None], axis=1), prefix, rank)
    return quantile_finish(prefix[:, 0::2], prefix[:, 1::2], frac, nan)


def blocks_to_csr(blockindex, d):
    """DEMCopt.blockindex (1-based ranges / index vectors, DEMC.jl:29) is given here as a list
    of 0-based index sequences; returns CSR (offsets, indices) as int32 arrays."""
    blocks = [np.asarray(list(b), dtype=np.int64) for b in blockindex]
    for b in blocks:
        if b.size == 0 or b.min() < 0 or b.max() >= d:
            raise ValueError("block indices must be 0-based and within [0, d)")
    offs = np.zeros(len(blocks) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([b.size for b in blocks])
    idx = np.concatenate(blocks).astype(np.int32)
    return offs, idx


class _PinnedOwner:
    """Pinned host buffers detached from a handle: returned to the library's pool when nothing refers to them any more."""

    def __init__(self, L, bases):
        self._L, self._bases = L, [b for b in bases if b]

    def __del__(self):
        try:
            for b in self._bases:
                self._L.demcz_release_host_buffer(C.c_void_p(b))
        except Exception:
            pass
        self._bases = []


class _HistoryStatistics:
    """The statistics over an on-device history, shared by everything that holds a handle with one: ``HipEngine`` (the history of
    a run) and ``DerivedHistory`` (functions of it).  Needs ``_L``, ``_h``, ``_chk``, ``N`` and ``d``."""

    def rhat(self, g_from, g_to):
        out = np.empty(self.d)
        self._chk(self._L.demcz_rhat(self._h, int(g_from), int(g_to), _lib.ptr(out)))
        return out

    def rhat_partial(self, g_from, g_to, stage, grand):
        out = np.empty(self.d if stage == 0 else 2 * self.d)
        g = _lib.f64(grand) if grand is not None else None
        self._chk(self._L.demcz_rhat_partial(self._h, int(g_from), int(g_to), int(stage), _lib.ptr(g), _lib.ptr(out)))
        return out

    def autocov_sums(self, g_from, g_to, lag_from, lag_to):
        """d x (lag_to - lag_from + 1): the sum over this engine's 2N split chains of n c_j(t) (demcz_autocov_sums)."""
        out = np.empty((self.d, max(0, int(lag_to) - int(lag_from) + 1)), order="F")
        self._chk(self._L.demcz_autocov_sums(self._h, int(g_from), int(g_to), int(lag_from), int(lag_to), _lib.ptr(out)))
        return out

    def ess(self, g_from, g_to, max_lag=0):
        """Effective sample size per parameter over generations g_from..g_to (demcz_ess): an ESS tuple."""
        d = self.d
        out = ESS(np.empty(d), np.empty(d), np.empty(d), np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int32))
        self._chk(self._L.demcz_ess(self._h, int(g_from), int(g_to), int(max_lag), _lib.ptr(out.ess), _lib.ptr(out.tau),
                                    _lib.ptr(out.varplus), _lib.ptr(out.pairs, _lib._lp), _lib.ptr(out.converged, _lib._ip)))
        return out

    def select_counts(self, g_from, g_to, shift, prefix):
        """One counting pass of the quantiles' radix select over this engine's chains (demcz_select_counts): prefix is (d, nprefix)
        uint64; returns (counts (d, nprefix, 256) int64, nan_count (d,) int64)."""
        prefix = np.array(prefix, dtype=np.uint64, order="F", ndmin=2)
        if prefix.shape[0] != self.d:
            raise ValueError("prefix must be (d, nprefix)")
        nprefix = prefix.shape[1]
        counts = np.zeros((self.d, nprefix, 256), dtype=np.int64)
        nan = np.zeros(self.d, dtype=np.int64)
        self._chk(self._L.demcz_select_counts(self._h, int(g_from), int(g_to), int(shift), nprefix, _lib.ptr(prefix, _lib._up),
                                              _lib.ptr(counts, _lib._lp), _lib.ptr(nan, _lib._lp)))
        return counts, nan

    def quantiles(self, g_from, g_to, probs, with_order_stats=False):
        """Quantiles per parameter over generations g_from..g_to (demcz_quantiles, Hyndman-Fan type 7, exact selection): d x nq,
        or a Quantiles tuple (q, lower, upper) with the two order statistics behind every entry."""
        probs = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
        nq, d = probs.size, self.d
        out = Quantiles(np.empty((d, nq), order="F"), np.empty((d, nq), order="F"), np.empty((d, nq), order="F"))
        self._chk(self._L.demcz_quantiles(self._h, int(g_from), int(g_to), nq, _lib.ptr(probs), _lib.ptr(out.q),
                                          _lib.ptr(out.lower), _lib.ptr(out.upper)))
        return out if with_order_stats else out.q

    def mean_cov(self, g_from, g_to):
        mean = np.empty(self.d)
        cov = np.empty((self.d, self.d), order="F")
        self._chk(self._L.demcz_mean_cov(self._h, int(g_from), int(g_to), _lib.ptr(mean), _lib.ptr(cov)))
        return mean, cov

    def derive(self, program, g_from, g_to):
        """``program`` (a ``DerivedProgram``) evaluated on every draw of generations g_from..g_to, on the device (demcz_derive):
        a ``DerivedHistory`` whose generations keep their numbers.  It owns its memory and outlives this object."""
        if program.d != self.d:
            raise ValueError("the program's d is not the history's")
        src, opts, data, ndata = program._args()
        out = C.c_void_p()
        self._chk(self._L.demcz_derive(self._h, int(g_from), int(g_to), program.m, src, opts, data, ndata, C.byref(out)))
        return DerivedHistory(self._L, out, self.N, program.m, int(g_from), int(g_to), program.names, getattr(self, "chain_id0", 0))

    def _stream_seed(self, seed):
        """The key of the draws' random streams: ``seed``, or the run's own where this object has one."""
        if seed is None:
            seed = getattr(self, "seed", None)
            if seed is None:
                raise ValueError("seed is required: this history does not know the seed of a run")
        return int(seed) & (2**64 - 1)

    def predict(self, program, g_from, g_to, seed=None):
        """``program`` (a ``PredictiveProgram``) at every draw of generations g_from..g_to, each draw with its own random stream
        keyed by (seed, generation, global chain) (demcz_predict): a ``DerivedHistory`` whose generations keep their numbers.
        ``seed``: default the engine's run seed (the streams cannot meet the sampler's); required on a ``DerivedHistory``."""
        if program.d != self.d:
            raise ValueError("the program's d is not the history's")
        seed = self._stream_seed(seed)
        src, opts, data, ndata = program._args()
        out = C.c_void_p()
        c0 = getattr(self, "chain_id0", 0)
        self._chk(self._L.demcz_predict(self._h, int(g_from), int(g_to), program.m, src, opts, data, ndata, seed, c0, C.byref(out)))
        return DerivedHistory(self._L, out, self.N, program.m, int(g_from), int(g_to), program.names, c0)

    def ppc(self, program, g_from, g_to, observed=None, seed=None):
        """The posterior predictive check of ``program`` (a ``PredictiveProgram``) over generations g_from..g_to (demcz_ppc): the
        calls ``predict`` makes, but only the counts of its m columns against ``observed`` (m values; None: zeros) leave the
        device -- a ``PPC`` record.  ``seed`` as for ``predict``."""
        if program.d != self.d:
            raise ValueError("the program's d is not the history's")
        seed = self._stream_seed(seed)
        obs = _ppc_observed(observed, program.m)
        src, opts, data, ndata = program._args()
        counts = np.zeros(3 * program.m, dtype=np.int64)
        self._chk(self._L.demcz_ppc(self._h, int(g_from), int(g_to), program.m, src, opts, data, ndata, seed, getattr(self, "chain_id0", 0),
                                    _lib.ptr(obs), _lib.ptr(counts, _lib._lp)))
        return ppc_record(counts, self.N * (int(g_to) - int(g_from) + 1), program.names)

    def rank_normalize(self, g_from, g_to, center=None, ranks=False):
        """The normal scores of the exact average ranks of every draw of generations g_from..g_to among all the window's draws of
        its parameter (demcz_rank_normalize): a ``DerivedHistory`` of d columns.  ``center`` (d values): rank
        ``fabs(x - center)`` instead of x (the folded form).  ``ranks``: the average ranks themselves."""
        ctr = None
        if center is not None:
            ctr = _lib.f64(center)
            if ctr.shape != (self.d,):
                raise ValueError("center must have d entries")
        out = C.c_void_p()
        self._chk(self._L.demcz_rank_normalize(self._h, int(g_from), int(g_to), 1 if ranks else 0, _lib.ptr(ctr), C.byref(out)))
        return DerivedHistory(self._L, out, self.N, self.d, int(g_from), int(g_to), getattr(self, "names", None), getattr(self, "chain_id0", 0))

    def indicator_le(self, g_from, g_to, thr):
        """The indicators x <= thr of every draw of generations g_from..g_to (demcz_indicator_le): ``thr`` is (d,) or (d, nthr); a
        ``DerivedHistory`` of d * nthr columns, column p + d * u holding parameter p against thr[p, u].  A NaN draw stays NaN."""
        thr = np.array(thr, dtype=np.float64, order="F")
        if thr.ndim == 1:
            thr = thr.reshape(-1, 1, order="F")
        if thr.ndim != 2 or thr.shape[0] != self.d:
            raise ValueError("thr must be (d,) or (d, nthr)")
        out = C.c_void_p()
        self._chk(self._L.demcz_indicator_le(self._h, int(g_from), int(g_to), thr.shape[1], _lib.ptr(thr), C.byref(out)))
        return DerivedHistory(self._L, out, self.N, self.d * thr.shape[1], int(g_from), int(g_to), None, getattr(self, "chain_id0", 0))

    def pointwise(self, program, g_from, g_to, obs_from=0, obs_to=None):
        """The log-likelihoods of observations obs_from .. obs_to - 1 (default: to the program's last; at most 32 of them) of
        ``program`` (a ``PointwiseProgram``) at every draw of generations g_from..g_to, on the device (demcz_pointwise): a
        ``DerivedHistory`` with one column per observation.  Its ``ess`` over the draws' ``N w`` gives an ``r_eff``."""
        if program.d != self.d:
            raise ValueError("the program's d is not the history's")
        obs_from = int(obs_from)
        obs_to = program.nobs if obs_to is None else int(obs_to)
        if not 0 <= obs_from < obs_to <= program.nobs:
            raise ValueError("need 0 <= obs_from < obs_to <= nobs")
        src, opts, data, ndata = program._args()
        out = C.c_void_p()
        self._chk(self._L.demcz_pointwise(self._h, int(g_from), int(g_to), obs_from, obs_to - obs_from, src, opts, data, ndata, C.byref(out)))
        names = None if program.names is None else program.names[obs_from:obs_to]
        return DerivedHistory(self._L, out, self.N, obs_to - obs_from, int(g_from), int(g_to), names, getattr(self, "chain_id0", 0))

    def loo_columns(self, g_from, g_to, r_eff=None):
        """PSIS-LOO and WAIC with the d columns of this history taken as the pointwise log-likelihoods of d observations over
        generations g_from..g_to (demcz_loo_columns): a ``LOO`` record.  ``r_eff``: a value or d values in (0, inf)."""
        e, k, n, l, w = _loo_outputs(self.d)
        r = _r_eff_arg(r_eff, self.d)
        self._chk(self._L.demcz_loo_columns(self._h, int(g_from), int(g_to), _lib.ptr(r), _lib.ptr(e), _lib.ptr(k), _lib.ptr(n, _lib._lp),
                                            _lib.ptr(l), _lib.ptr(w)))
        return loo_record(e, k, n, l, w, self.N * (int(g_to) - int(g_from) + 1), getattr(self, "names", None))

    def loo(self, program, g_from, g_to, r_eff=None):
        """PSIS-LOO and WAIC of ``program`` (a ``PointwiseProgram``) over generations g_from..g_to (demcz_loo): the observations
        are evaluated, reduced and dropped in chunks on the device; a ``LOO`` record.  ``r_eff``: a value or nobs values."""
        if program.d != self.d:
            raise ValueError("the program's d is not the history's")
        nobs = program.nobs
        e, k, n, l, w = _loo_outputs(nobs)
        r = _r_eff_arg(r_eff, nobs)
        src, opts, data, ndata = program._args()
        self._chk(self._L.demcz_loo(self._h, int(g_from), int(g_to), nobs, src, opts, data, ndata, _lib.ptr(r), _lib.ptr(e), _lib.ptr(k),
                                    _lib.ptr(n, _lib._lp), _lib.ptr(l), _lib.ptr(w)))
        return loo_record(e, k, n, l, w, self.N * (int(g_to) - int(g_from) + 1), program.names)

    def rank_diagnostics(self, g_from, g_to):
        """Rank-normalised split R-hat, bulk-ESS and tail-ESS per parameter over generations g_from..g_to (demcz_rank_diagnostics):
        a RankDiagnostics tuple."""
        out = RankDiagnostics(np.empty(self.d), np.empty(self.d), np.empty(self.d))
        self._chk(self._L.demcz_rank_diagnostics(self._h, int(g_from), int(g_to), _lib.ptr(out.rhat_rank), _lib.ptr(out.ess_bulk),
                                                 _lib.ptr(out.ess_tail)))
        return out

    def histogram(self, g_from, g_to, bins=33, range=None):
        """Marginal histograms of every parameter over generations g_from..g_to (demcz_histogram): a ``Histogram``.  ``bins``: 1 to
        4096 uniform bins; ``range``: (lo, hi) for every parameter, d x 2, or None: the window's smallest and largest draw of each
        parameter (a parameter with a NaN or infinite draw then needs a range).  The counts are np.histogram's."""
        d, nb = self.d, int(bins)
        lo, hi = _range_args(range, d)
        out = Histogram(np.zeros((d, max(nb, 0)), dtype=np.int64), np.empty((d, max(nb, 0) + 1)), np.zeros(d, dtype=np.int64),
                        np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int64))
        self._chk(self._L.demcz_histogram(self._h, int(g_from), int(g_to), nb, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(out.edges),
                                          _lib.ptr(out.counts, _lib._lp), _lib.ptr(out.below, _lib._lp), _lib.ptr(out.above, _lib._lp),
                                          _lib.ptr(out.nan, _lib._lp)))
        return out

    def histogram2d(self, g_from, g_to, pairs=None, bins=32, range=None):
        """Pairwise histograms over generations g_from..g_to (demcz_histogram2d): a ``Histogram2D``.  ``pairs``: (p, q) pairs with
        p != q (default: all p < q); ``bins``: one number or (nbx, nby), each 1 to 128; ``range`` as for ``histogram``.  The counts
        of pair (p, q) are np.histogram2d(x_p, x_q, bins=[edges_x[p], edges_y[q]])'s."""
        d = self.d
        nbx, nby = _bins2(bins)
        pr = _pairs_arg(pairs, d)
        lo, hi = _range_args(range, d)
        npairs = pr.shape[0]
        counts = np.zeros((npairs, max(nbx, 0), max(nby, 0)), dtype=np.int64)
        ex, ey = np.empty((d, max(nbx, 0) + 1)), np.empty((d, max(nby, 0) + 1))
        outside = np.zeros(npairs, dtype=np.int64)
        self._chk(self._L.demcz_histogram2d(self._h, int(g_from), int(g_to), npairs, _lib.ptr(pr, _lib._ip), nbx, nby, _lib.ptr(lo),
                                            _lib.ptr(hi), _lib.ptr(ex), _lib.ptr(ey), _lib.ptr(counts, _lib._lp),
                                            _lib.ptr(outside, _lib._lp)))
        return Histogram2D(counts, pr, (ex, ey), outside)

    def hdi(self, g_from, g_to, prob=0.94):
        """The highest-density interval of every parameter over generations g_from..g_to (demcz_hdi): the shortest interval between
        two order statistics that spans floor(prob S) steps among the S sorted draws (ArviZ's unimodal hdi).  d x 2, or
        d x nprob x 2 for several probabilities (up to 16).  ``Histogram.hdi`` has the multimodal one."""
        probs = np.ascontiguousarray(np.atleast_1d(prob), dtype=np.float64)
        out = np.empty((self.d, probs.size, 2))
        self._chk(self._L.demcz_hdi(self._h, int(g_from), int(g_to), probs.size, _lib.ptr(probs), _lib.ptr(out)))
        return out[:, 0, :] if np.ndim(prob) == 0 else out


class DerivedHistory(_HistoryStatistics):
    """An N x m x w history of derived quantities on the device (``demcz_derive``): generations ``g_from..g_to``, numbered as in
    the history it came from.  ``rhat``, ``rhat_partial``, ``autocov_sums``, ``ess``, ``select_counts``, ``quantiles``, ``mean_cov``,
    ``derive``, ``predict``, ``ppc``, ``rank_normalize``, ``indicator_le``, ``rank_diagnostics``, ``histogram``, ``histogram2d``, ``hdi``, ``pointwise``, ``loo_columns`` and ``loo`` are ``HipEngine``'s; nothing else of an engine applies (the library answers ERR_STATE)."""

    def __init__(self, L, handle, N, m, g_from, g_to, names=None, chain_id0=0):
        self._L, self._h = L, handle
        self.N, self.d, self.m = int(N), int(m), int(m)
        self.g_from, self.g_to = int(g_from), int(g_to)
        self.names = list(names) if names is not None else None
        self.chain_id0 = int(chain_id0)

    def _chk(self, rc):
        if rc != 0:
            raise DemczError(rc, (self._L.demcz_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.demcz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def synchronize(self):
        self._chk(self._L.demcz_synchronize(self._h))

    def get(self, g_from=None, g_to=None):
        """The values of generations g_from..g_to (default: all) as an N x m x w column-major array."""
        g_from = self.g_from if g_from is None else int(g_from)
        g_to = self.g_to if g_to is None else int(g_to)
        out = np.empty((self.N, self.m, max(0, g_to - g_from + 1)), order="F")
        self._chk(self._L.demcz_get_history(self._h, g_from, g_to, _lib.ptr(out), None))
        return out

    def summary(self, probs=None, rank_normalized=False, hdi_prob=None):
        """What ``posterior_summary`` returns for a host array (mean, sd, mcse, ess, rhat, converged and, with ``probs``,
        quantiles; with ``rank_normalized``, rhat_rank, ess_bulk and ess_tail; with ``hdi_prob``, hdi), computed from the handle
        with no download, plus ``names``."""
        mean, _ = self.mean_cov(self.g_from, self.g_to)
        e = self.ess(self.g_from, self.g_to)
        with np.errstate(all="ignore"):
            out = dict(mean=mean, sd=np.sqrt(e.varplus), mcse=np.sqrt(e.varplus / e.ess), ess=e.ess,
                       rhat=self.rhat(self.g_from, self.g_to), converged=e.converged)
        if probs is not None:
            out["quantiles"] = self.quantiles(self.g_from, self.g_to, probs)
        if rank_normalized:
            out.update(self.rank_diagnostics(self.g_from, self.g_to)._asdict())
        if hdi_prob is not None:
            out["hdi"] = self.hdi(self.g_from, self.g_to, hdi_prob)
        out["names"] = self.names
        return out


class HipEngine(_HistoryStatistics):
    """Device state of one shard: Z replica, current states, history, RNG position."""

    def __init__(self, *, N, d, K, Mcap, Gcap, blockindex, eps_scale, seed, target, chain_id0=0,
                 device_id=0, stream=None, lanes_per_chain=0):
        self._L = _lib.load()
        self.N, self.d, self.K, self.Mcap, self.Gcap = int(N), int(d), int(K), int(Mcap), int(Gcap)
        self.chain_id0 = int(chain_id0)
        self.seed = int(seed) & (2**64 - 1)
        self._keep = []
        offs, idx = blocks_to_csr(blockindex, d)
        eps = _lib.f64(eps_scale)
        if eps.shape != (d,):
            raise ValueError("eps_scale must have d entries")
        self._keep += [offs, idx, eps]
        cfg = _lib.Config()
        cfg.N, cfg.chain_id0, cfg.d, cfg.K = self.N, self.chain_id0, self.d, self.K
        cfg.Mcap, cfg.Gcap, cfg.Nblocks = self.Mcap, self.Gcap, len(offs) - 1
        cfg.block_offsets, cfg.block_indices = _lib.ptr(offs, _lib._ip), _lib.ptr(idx, _lib._ip)
        cfg.eps_scale, cfg.seed, cfg.device_id = _lib.ptr(eps), int(seed) & (2**64 - 1), int(device_id)
        cfg.stream = stream
        cfg.lanes_per_chain = int(lanes_per_chain)
        if is_device_target(target):
            if target.d != d:
                raise ValueError("target dimension != d")
            cfg.target_kind = target.kind
            target.fill(cfg, self._keep)
        elif callable(target):
            cfg.target_kind = _lib.TARGET_HOST_CALLBACK
        else:
            raise TypeError("target must be a device target or a callable")
        self.host_callback = cfg.target_kind == _lib.TARGET_HOST_CALLBACK
        self._h = C.c_void_p()
        rc = self._L.demcz_create(C.byref(self._h), C.byref(cfg))
        if rc != 0:
            raise DemczError(rc, (self._L.demcz_last_error(None) or b"").decode())
        if cfg.target_kind == _lib.TARGET_PROGRAM:
            try:
                self._chk(target.attach(self._L, self._h))
            except DemczError:
                self.close()
                raise

    # -- plumbing -----------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise DemczError(rc, (self._L.demcz_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.demcz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the marginal likelihood (demcz_bridge) ------------------------------------------------
    def bridge_posterior(self, g_from, g_to, mean, L):
        """a1 = log_obj - log g(x) of every draw of generations g_from..g_to, g = N(mean, L L^T) (demcz_bridge_posterior): a
        one-column ``DerivedHistory`` (a context manager) whose generations keep their numbers."""
        mean, L = _bridge_ml(mean, L, self.d)
        out = C.c_void_p()
        self._chk(self._L.demcz_bridge_posterior(self._h, int(g_from), int(g_to), _lib.ptr(mean), _lib.ptr(L), C.byref(out)))
        return DerivedHistory(self._L, out, self.N, 1, int(g_from), int(g_to), ["a1"], self.chain_id0)

    def bridge_proposal(self, Np, wp, mean, L, seed=None, want_draws=False):
        """Np x wp fresh draws of g = N(mean, L L^T) and a2 = logobj(x) - log g(x) with this engine's own target
        (demcz_bridge_proposal): a one-column ``DerivedHistory`` of generations 1..wp, or with ``want_draws`` the pair (a2, draws),
        draws an Np x d x wp ``DerivedHistory``.  ``seed``: default ``bridge_seed(self.seed)``."""
        mean, L = _bridge_ml(mean, L, self.d)
        seed = bridge_seed(self.seed) if seed is None else int(seed) & (2**64 - 1)
        a2, xs = C.c_void_p(), C.c_void_p()
        self._chk(self._L.demcz_bridge_proposal(self._h, int(Np), int(wp), seed, _lib.ptr(mean), _lib.ptr(L), C.byref(a2),
                                                C.byref(xs) if want_draws else None))
        ha = DerivedHistory(self._L, a2, int(Np), 1, 1, int(wp), ["a2"])
        return (ha, DerivedHistory(self._L, xs, int(Np), self.d, 1, int(wp), getattr(self, "names", None))) if want_draws else ha

    def bridge(self, g_from, g_to, seed=None, neff="auto", tol=1e-10, max_iter=1000):
        """The marginal likelihood log Z = log integral exp(logobj) by bridge sampling over generations g_from..g_to (demcz_bridge):
        a ``Bridge`` record.  The first half of the window fits a normal proposal, the second half is iterated against as many
        fresh draws of it.  ``neff``: the effective number of posterior draws; "auto" is the median over the parameters of
        ``ess`` of the iteration window, None all N1 of them.  ``seed``: the proposal's streams; the default is
        ``bridge_seed(self.seed)``, the run's seed XOR ``BRIDGE_SEED_XOR`` -- with the run's own seed the proposal would replay
        the sampler's streams.  Assumes that log_obj is the untempered log-posterior and that the window is converged; a
        posterior far from normal shows as a large ``se_logml`` and a slow iteration."""
        g_from, g_to = int(g_from), int(g_to)
        if isinstance(neff, str):
            if neff != "auto":
                raise ValueError('neff must be a number, None or "auto"')
            w = g_to - g_from + 1
            ne = float(np.median(self.ess(g_from + w // 2, g_to).ess)) if w >= 8 else 0.0
            ne = ne if np.isfinite(ne) and ne > 0 else 0.0
        else:
            ne = 0.0 if neff is None else float(neff)
        seed = bridge_seed(self.seed) if seed is None else int(seed) & (2**64 - 1)
        o = _bridge_outputs(self.d)
        self._chk(self._L.demcz_bridge(self._h, g_from, g_to, seed, ne, float(tol), int(max_iter), *_bridge_out_args(o)))
        return _bridge_record(o)

    # -- state --------------------------------------------------------------------------------
    def set_state(self, X, logp, Z):
        X = _lib.f64(X, "F")
        Z = _lib.f64(Z, "F")
        if X.shape != (self.N, self.d) or Z.ndim != 2 or Z.shape[1] != self.d:
            raise ValueError("X must be N x d and Z must be M0 x d")
        lp = _lib.f64(logp) if logp is not None else None
        if lp is not None and lp.shape != (self.N,):
            raise ValueError("logp must have N entries")
        self._chk(self._L.demcz_set_state(self._h, _lib.ptr(X), _lib.ptr(lp), _lib.ptr(Z), Z.shape[0], Z.shape[0]))

    def get_state(self, with_Z=True):
        X = np.empty((self.N, self.d), order="F")
        lp = np.empty(self.N)
        M = C.c_int64()
        self._chk(self._L.demcz_get_state(self._h, _lib.ptr(X), _lib.ptr(lp), None, 0, C.byref(M)))
        Z = None
        if with_Z:
            # the archive comes back in a pinned buffer of the library's pool (no page faults of a fresh 41 MB array under the
            # copy); the array below is a view of it, and the buffer returns to the pool with the array
            pz, Mz = C.c_void_p(), C.c_int64()
            self._chk(self._L.demcz_get_archive_pinned(self._h, C.byref(pz), C.byref(Mz)))
            buf = (C.c_double * (Mz.value * self.d)).from_address(pz.value)
            buf._owner = _PinnedOwner(self._L, [pz.value])
            Z = np.ctypeslib.as_array(buf).reshape((Mz.value, self.d), order="F")
        return X, lp, Z, int(M.value)

    @property
    def M(self):
        M = C.c_int64()
        self._chk(self._L.demcz_get_info(self._h, C.byref(M), None, None))
        return int(M.value)

    def info(self):
        M, nl, lanes = C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self._L.demcz_get_info(self._h, C.byref(M), C.byref(nl), C.byref(lanes)))
        return dict(M=int(M.value), window_launches=int(nl.value), lanes_per_chain=int(lanes.value))

    def set_append_lag(self, batches):
        self._chk(self._L.demcz_set_append_lag(self._h, int(batches)))

    def set_rng_offset(self, generations):
        self._chk(self._L.demcz_set_rng_offset(self._h, int(generations)))

    def set_snooker(self, every, gamma=(1.2, 2.2)):
        """demcz_set_snooker: every ``every``-th generation (of the stream numbering) is a snooker generation with
        gamma_s ~ U(gamma[0], gamma[1]); 0 switches them off.  One-lane handles (``lanes_per_chain=1``) only."""
        lo, hi = gamma
        self._chk(self._L.demcz_set_snooker(self._h, C.c_int32(int(every)), C.c_double(float(lo)), C.c_double(float(hi))))

    @property
    def snooker(self):
        """(every, gamma_lo, gamma_hi, snooker launches made so far) -- demcz_get_snooker."""
        ev, lo, hi, n = C.c_int32(0), C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        self._chk(self._L.demcz_get_snooker(self._h, C.byref(ev), C.byref(lo), C.byref(hi), C.byref(n)))
        return int(ev.value), float(lo.value), float(hi.value), int(n.value)

    def set_crossover(self, ncr=3, delta_max=3, weights=None):
        """demcz_set_crossover: with ``ncr >= 1`` every generation that is not a snooker generation is a crossover generation of
        DREAM(ZS) -- each chain moves a random subset of its parameters (CR class m of ``ncr``, drawn with the integer
        ``weights``, selects a parameter with probability (m + 1) / ncr) by the sum of 1 ... ``delta_max`` archive differences,
        one log-density evaluation a generation.  ``ncr=0`` switches off.  One-lane handles (``lanes_per_chain=1``) with one
        block, before the first generation (and before ``set_rng_offset`` on a resumed run)."""
        ncr = int(ncr)
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.int32)
            if w.shape != (ncr,):
                raise ValueError("weights: one integer per CR class")
            wp = w.ctypes.data_as(C.POINTER(C.c_int32))
        self._chk(self._L.demcz_set_crossover(self._h, C.c_int32(ncr), wp, C.c_int32(int(delta_max))))

    @property
    def crossover(self):
        """``Crossover(ncr, delta_max, weights, tried, accepted)`` -- demcz_get_crossover; ``tried`` and ``accepted`` are the
        steps per CR class over the handle's life (arrays of length ncr), ``.accept_rate`` their ratio."""
        n, dm = C.c_int32(0), C.c_int32(0)
        w, tr, ac = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        self._chk(self._L.demcz_get_crossover(self._h, C.byref(n), w.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(dm),
                                              tr.ctypes.data_as(C.POINTER(C.c_int64)), ac.ctypes.data_as(C.POINTER(C.c_int64))))
        k = int(n.value)
        return Crossover(k, int(dm.value), w[:k].copy(), tr[:k].copy(), ac[:k].copy())

    def set_crossover_adapt(self, every, until, min_weight=656):
        """demcz_set_crossover_adapt: adapt the CR class weights during burn-in, on the device (DREAM's rule).  Up to the position
        ``until`` (a multiple of ``every``; positions count as the snooker rule's, ``g + rng_offset``) every accepted crossover
        step adds its squared jump distance, normalised by the spread of the chains, to its class; behind every ``every``-th
        generation the weights become proportional to the jump distance per step tried, no smaller than ``min_weight`` of 65536.
        ``every=0`` switches off.  On a fresh crossover handle that does not append externally; ``N * until < 2**31``."""
        self._chk(self._L.demcz_set_crossover_adapt(self._h, C.c_int64(int(every)), C.c_int64(int(until)), C.c_int32(int(min_weight))))

    @property
    def crossover_adapt(self):
        """``CrossoverAdapt(every, until, min_weight, weights, dist, tried, rsd, updates)`` -- demcz_get_crossover_adapt (arrays of
        length ncr, ``rsd`` of length d); ``.jump_per_try`` and ``.shares``.  Synchronises the handle's stream."""
        ev, un, mw, up = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)
        w, di, tr = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        rsd = np.zeros(self.d, dtype=np.float64)
        self._chk(self._L.demcz_get_crossover_adapt(self._h, C.byref(ev), C.byref(un), C.byref(mw), w.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    di.ctypes.data_as(C.POINTER(C.c_int64)), tr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    rsd.ctypes.data_as(C.POINTER(C.c_double)), C.byref(up)))
        k = self.crossover.ncr
        return CrossoverAdapt(int(ev.value), int(un.value), int(mw.value), w[:k].copy(), di[:k].copy(), tr[:k].copy(), rsd, int(up.value))

    def set_crossover_adapt_state(self, weights, dist, tried, rsd, updates):
        """demcz_set_crossover_adapt_state: the state ``crossover_adapt`` returned, onto a fresh handle with the adaptation set --
        the other half of a checkpoint (with ``set_rng_offset`` the run continues as the uninterrupted one)."""
        k = self.crossover.ncr
        w, di, tr = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        if not (len(weights) == len(dist) == len(tried) == k):
            raise ValueError("weights, dist, tried: one value per CR class")
        w[:k], di[:k], tr[:k] = weights, dist, tried
        r = np.ascontiguousarray(rsd, dtype=np.float64)
        if r.shape != (self.d,):
            raise ValueError("rsd: one value per parameter")
        self._chk(self._L.demcz_set_crossover_adapt_state(self._h, w.ctypes.data_as(C.POINTER(C.c_int32)), di.ctypes.data_as(C.POINTER(C.c_int64)),
                                                          tr.ctypes.data_as(C.POINTER(C.c_int64)), r.ctypes.data_as(C.POINTER(C.c_double)),
                                                          C.c_int64(int(updates))))

    def set_crossover_weights(self, weights):
        """demcz_set_crossover_weights: new class weights for a crossover handle in mid-life (from the next launch on); refused
        while the adaptation is still running."""
        w = np.ascontiguousarray(weights, dtype=np.int32)
        if w.shape != (self.crossover.ncr,):
            raise ValueError("weights: one integer per CR class")
        self._chk(self._L.demcz_set_crossover_weights(self._h, w.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_history_origin(self, g0):
        self._chk(self._L.demcz_set_history_origin(self._h, int(g0)))

    # -- the hot path -------------------------------------------------------------------------
    def run(self, g_from, g_to, gamma, temperature=None):
        t = None
        if temperature is not None:
            t = _lib.f64(temperature)
            if t.shape != (g_to - g_from + 1,):
                raise ValueError("one temperature per generation")
        self._chk(self._L.demcz_run(self._h, int(g_from), int(g_to), float(gamma), _lib.ptr(t)))

    def run_checked(self, g_from, g_to, gamma, every, threshold=0.0, temperature=None):
        """demcz_run_checked: the generation loop with its R-hat test every ``every`` generations as one
        library call (demcz.jl:30-55).  Returns (g_stop, max R-hat of every check made, R-hat vector of the last)."""
        t = None
        if temperature is not None:
            t = _lib.f64(temperature)
            if t.shape != (g_to - g_from + 1,):
                raise ValueError("one temperature per generation")
        n_max = int((g_to - g_from + 1) // every + 2)
        mx = np.zeros(n_max)
        last = np.full(self.d, np.nan)
        g_stop, n = C.c_int64(0), C.c_int32(0)
        self._chk(self._L.demcz_run_checked(self._h, C.c_int64(int(g_from)), C.c_int64(int(g_to)), C.c_double(float(gamma)),
                                            _lib.ptr(t), C.c_int64(int(every)), C.c_double(float(threshold)), C.byref(g_stop),
                                            C.byref(n), _lib.ptr(mx), C.c_int32(n_max), _lib.ptr(last)))
        return int(g_stop.value), mx[:n.value].copy(), last

    def set_kernel_timing(self, enabled: bool):
        self._chk(self._L.demcz_set_kernel_timing(self._h, C.c_int32(1 if enabled else 0)))

    def get_kernel_time(self):
        """(launches, milliseconds) of the window kernels timed since the last call (HIP events on the kernel's stream)."""
        n, ms = C.c_int64(0), C.c_double(0.0)
        self._chk(self._L.demcz_get_kernel_time(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def get_kernel_time_series(self):
        """(start_ms, duration_ms) arrays of the brackets the last get_kernel_time() summed up, one entry per autostop slab: a
        bracket over k slabs that run_checked made one demcz_run call of comes back as k equal shares (means, not events)."""
        n = C.c_int32(0)
        self._chk(self._L.demcz_get_kernel_time_series(self._h, 0, None, None, C.byref(n)))
        st, du = np.zeros(n.value), np.zeros(n.value)
        self._chk(self._L.demcz_get_kernel_time_series(self._h, n.value, _lib.ptr(st), _lib.ptr(du), C.byref(n)))
        return st, du

    def set_live_spin_limit(self, polls: int):
        """Diagnostic: polls before a LIVE row wait gives up (tests force the fall-back path with 1)."""
        self._chk(self._L.demcz_set_live_spin_limit(self._h, C.c_int32(int(polls))))

    def debug_set_live_fault(self, polls: int, g_from: int = 0):
        """Diagnostic: LIVE launches starting at generation g_from or later use the poll limit `polls` (0: off)."""
        self._chk(self._L.demcz_debug_set_live_fault(self._h, C.c_int32(int(polls)), C.c_int64(int(g_from))))

    def live_status(self):
        """Diagnostic: (LIVE launches in use, number of fall-backs to one launch per K-window)."""
        on, redos = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.demcz_get_live_status(self._h, C.byref(on), C.byref(redos)))
        return bool(on.value), int(redos.value)

    def set_live_rearms(self, n: int):
        """How many more times the handle may go back to LIVE launches after a failed hand-off (default 3; 0: a failure leaves
        it at one launch per K-window for good, the behaviour of rounds 2-4)."""
        self._chk(self._L.demcz_set_live_rearms(self._h, C.c_int32(int(n))))

    def live_rearms(self):
        """Diagnostic: (times the handle went LIVE again after a fall-back, re-arms left)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.demcz_get_live_rearms(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kernel_counts(self):
        """Diagnostic: window launches so far by kernel -- {"ps2", "ps_general", "other"} (demcz_debug_kernel_counts)."""
        c = (C.c_int64 * 3)()
        self._chk(self._L.demcz_debug_kernel_counts(self._h, c))
        return dict(zip(("ps2", "ps_general", "other"), (int(v) for v in c)))

    def kernel_name(self):
        """Diagnostic: the window kernel the most recent window launch ran, as a profiler names it."""
        buf = C.create_string_buffer(192)
        self._chk(self._L.demcz_debug_kernel_name(self._h, buf, 192))
        return buf.value.decode()

    def synchronize(self):
        self._chk(self._L.demcz_synchronize(self._h))

    # -- results ------------------------------------------------------------------------------
    def get_history(self, g_from, g_to, chain=True, log_obj=True, out=None):
        """`out`: (chain, log_obj) column-major arrays of at least g_to - g_from + 1 generations to fill instead of new ones
        (their pages already touched: the download then runs at the link's rate, not at the page faults'); the views of
        the generations asked for are returned."""
        G = g_to - g_from + 1
        if out is not None and chain and log_obj:
            ch_full, lo_full = out
            ok = (ch_full.flags.f_contiguous and lo_full.flags.f_contiguous and ch_full.shape[:2] == (self.N, self.d)
                  and lo_full.shape[0] == self.N and ch_full.shape[2] >= G and lo_full.shape[1] >= G
                  and ch_full.dtype == np.float64 and lo_full.dtype == np.float64)
            if ok:
                self._chk(self._L.demcz_get_history(self._h, int(g_from), int(g_to), _lib.ptr(ch_full), _lib.ptr(lo_full)))
                return ch_full[:, :, :G], lo_full[:, :G]
        ch = np.empty((self.N, self.d, G), order="F") if chain else None
        lo = np.empty((self.N, G), order="F") if log_obj else None
        self._chk(self._L.demcz_get_history(self._h, int(g_from), int(g_to), _lib.ptr(ch), _lib.ptr(lo)))
        return ch, lo

    # -- streamed history: pinned host mirrors filled while the GPU runs (demcz_history_stream) -------------------------
    def history_stream(self, enabled=True):
        self._chk(self._L.demcz_history_stream(self._h, 1 if enabled else 0))
        self._streaming = bool(enabled)

    def take_history(self, g_from, g_to):
        """mc.chain[:, :, g_from:g_to], mc.log_obj[:, g_from:g_to] as NumPy arrays OVER the library's pinned mirrors (no copy):
        the mirrors are detached from the handle and go back to the library's pool when the last array over them is
        collected.  One call per run (the handle keeps no mirrors afterwards)."""
        G = g_to - g_from + 1
        pc, pl = C.c_void_p(), C.c_void_p()
        self._chk(self._L.demcz_get_history_view(self._h, int(g_from), int(g_to), C.byref(pc), C.byref(pl)))
        bc, bl = C.c_void_p(), C.c_void_p()
        self._chk(self._L.demcz_detach_history(self._h, C.byref(bc), C.byref(bl)))
        self._streaming = False
        owner = _PinnedOwner(self._L, [bc.value, bl.value])
        cbuf = (C.c_double * (self.N * self.d * G)).from_address(pc.value)
        lbuf = (C.c_double * (self.N * G)).from_address(pl.value)
        cbuf._owner = owner          # (NumPy keeps the ctypes object alive; the ctypes object keeps the owner alive)
        lbuf._owner = owner
        chain = np.ctypeslib.as_array(cbuf).reshape((self.N, self.d, G), order="F")
        lobj = np.ctypeslib.as_array(lbuf).reshape((self.N, G), order="F")
        return chain, lobj

    def get_changed(self, g_from, g_to):
        out = np.zeros(g_to - g_from + 1, dtype=np.int64)
        self._chk(self._L.demcz_get_changed(self._h, int(g_from), int(g_to), _lib.ptr(out, _lib._lp)))
        return out

    def changed_total(self, g_from, g_to, with_source=False):
        """Sum of get_changed over g_from..g_to, from the window kernels' ballot counters when the range is made of
        whole launches (demcz_get_changed_total).  with_source: also return whether the ballots answered."""
        tot, src = C.c_int64(0), C.c_int32(0)
        self._chk(self._L.demcz_get_changed_total(self._h, int(g_from), int(g_to), C.byref(tot), C.byref(src)))
        return (int(tot.value), bool(src.value)) if with_source else int(tot.value)

    def best(self, g_from, g_to):
        """The best draw of generations g_from..g_to (demcz_best): a Best tuple; chain is 0-based and local to this engine."""
        v, c, g = C.c_double(), C.c_int64(), C.c_int64()
        par = np.empty(self.d)
        self._chk(self._L.demcz_best(self._h, int(g_from), int(g_to), C.byref(v), C.byref(c), C.byref(g), _lib.ptr(par)))
        return Best(v.value, c.value, g.value, par)

    def accept_ratio(self, g_from, g_to):
        out = np.empty(self.N)
        self._chk(self._L.demcz_accept_ratio(self._h, int(g_from), int(g_to), _lib.ptr(out)))
        return out

    # -- host-closure mode ----------------------------------------------------------------------
    def closure_buffers(self):
        """demcz_closure_buffers: (Xprop, logp) NumPy views of the handle's pinned host buffers -- N x d column-major and N.
        After this call propose() returns a view of Xprop (no copy, no stream synchronisation) and accept_commit() with no
        argument commits whatever has been written into logp."""
        if getattr(self, "_hc", None) is None:
            px, pl = C.c_void_p(), C.c_void_p()
            self._chk(self._L.demcz_closure_buffers(self._h, C.byref(px), C.byref(pl)))
            bx = (C.c_double * (self.N * self.d)).from_address(px.value)
            bl = (C.c_double * self.N).from_address(pl.value)
            self._hc = (np.ctypeslib.as_array(bx).reshape((self.N, self.d), order="F"), np.ctypeslib.as_array(bl))
        return self._hc

    def propose(self, g, ib, gamma):
        if getattr(self, "_hc", None) is not None:
            self._chk(self._L.demcz_propose(self._h, int(g), int(ib), float(gamma), None))
            return self._hc[0]
        Xp = np.empty((self.N, self.d), order="F")
        self._chk(self._L.demcz_propose(self._h, int(g), int(ib), float(gamma), _lib.ptr(Xp)))
        return Xp

    def accept_commit(self, logp_prop=None, temperature=None):
        t = C.byref(C.c_double(float(temperature))) if temperature is not None else None
        tp = C.cast(t, _lib._dp) if t is not None else None
        hc = getattr(self, "_hc", None)
        if logp_prop is None or (hc is not None and logp_prop is hc[1]):
            if hc is None:
                raise ValueError("accept_commit() without values needs closure_buffers() first")
            self._chk(self._L.demcz_accept_commit(self._h, None, tp))
            return
        lp = _lib.f64(logp_prop)
        self._chk(self._L.demcz_accept_commit(self._h, _lib.ptr(lp), tp))

    def end_generation(self, g):
        self._chk(self._L.demcz_end_generation(self._h, int(g)))

    # -- multi-GPU ------------------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self._L.demcz_comm_unique_id(buf)
        if rc != 0:
            raise DemczError(rc, (self._L.demcz_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        buf = C.create_string_buffer(unique_id, 128)
        self._chk(self._L.demcz_comm_init(self._h, buf, int(nranks), int(rank)))

    @staticmethod
    def peer_group(engines):
        """demcz_peer_group: the engines (shards of one run, all in this process on one device) publish their K-boundary rows
        into each other's archive replicas from inside their launches."""
        L = engines[0]._L
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        rc = L.demcz_peer_group(arr, len(engines))
        if rc != 0:
            msgs = [(L.demcz_last_error(e._h) or b"").decode() for e in engines]
            raise DemczError(rc, next((m for m in msgs if m), ""))

    def peer_export(self, nranks: int, rank: int) -> bytes:
        """demcz_peer_export: the archive becomes fine-grained, IPC-exportable memory; returns its 64-byte handle."""
        buf = C.create_string_buffer(64)
        self._chk(self._L.demcz_peer_export(self._h, int(nranks), int(rank), buf))
        return buf.raw

    def peer_attach(self, handles):
        """demcz_peer_attach: `handles` = the 64-byte handles of all ranks in rank order (this rank's own included)."""
        blob = b"".join(handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._chk(self._L.demcz_peer_attach(self._h, buf))

    def peer_detach(self):
        """demcz_peer_detach (host-mediated IPC peers): close this rank's mappings of the other ranks' archives.  Call between
        two barriers of the host's, after the last run and before any rank closes its engine."""
        self._chk(self._L.demcz_peer_detach(self._h))

    def peer_ping(self):
        """(ok, wait_us) of demcz_comm_init's first-contact check: ok = 1 passed on all ranks, 0 failed somewhere (the run
        exchanges through ncclAllGather), -1 not made; wait_us = how long this rank waited for the last peer's token."""
        ok, us = C.c_int32(-1), C.c_double(0.0)
        self._chk(self._L.demcz_get_peer_ping(self._h, C.byref(ok), C.byref(us)))
        return int(ok.value), float(us.value)

    def peer_status(self):
        """(mode, peers): mode 0 = RCCL exchange or unsharded, 1 = replica group of this process (demcz_peer_group), 2 = IPC
        peers set up over the library's communicator (demcz_comm_init), 3 = IPC peers set up by the host carrying the handles
        (demcz_peer_export / demcz_peer_attach: no automatic redo, the host owes the barriers); peers = replicas this handle
        publishes into besides its own."""
        m, n = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.demcz_get_peer_status(self._h, C.byref(m), C.byref(n)))
        return int(m.value), int(n.value)

    def set_comm_timeout(self, milliseconds: int):
        """Deadline of every host-side wait of a sharded handle; past it the communicators are aborted and calls raise
        DemczError with code ERR_COMM (0 = wait for ever)."""
        self._chk(self._L.demcz_set_comm_timeout(self._h, C.c_int64(int(milliseconds))))

    def debug_stall_exchange(self, milliseconds: int):
        """Diagnostic: hold the next collective back on its stream for `milliseconds` (what a stalled peer looks like)."""
        self._chk(self._L.demcz_debug_stall_exchange(self._h, C.c_int32(int(milliseconds))))

    def set_external_append(self, enabled: bool):
        self._chk(self._L.demcz_set_external_append(self._h, 1 if enabled else 0))

    def append_rows(self, rows):
        rows = _lib.f64(rows, "F")
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError("rows must be nrows x d")
        self._chk(self._L.demcz_append_rows(self._h, _lib.ptr(rows), rows.shape[0], rows.shape[0]))

    def debug_append_slab(self, slab, R, cnt, batched):
        """Diagnostic: run the sharded exchange's scatter kernel on a caller-built [R][cnt][d][N] slab."""
        slab = _lib.f64(slab)
        if slab.size != R * cnt * self.d * self.N:
            raise ValueError("slab must hold R*cnt*d*N doubles")
        self._chk(self._L.demcz_debug_append_slab(self._h, _lib.ptr(slab), int(R), int(cnt), 1 if batched else 0))

    def export_current_device(self, device_ptr: int):
        self._chk(self._L.demcz_export_current_device(self._h, C.c_void_p(device_ptr)))

    def append_rows_device(self, device_ptr: int, nrows: int, ldrows: int):
        self._chk(self._L.demcz_append_rows_device(self._h, C.c_void_p(device_ptr), int(nrows), int(ldrows)))


def pool_trim():
    """Give the buffers the library keeps for the next handle back to the runtime: (device bytes, pinned bytes) freed."""
    L = _lib.load()
    a, b = C.c_int64(0), C.c_int64(0)
    L.demcz_pool_trim(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def selftest_draws(seed, chain, blk0, n, device_id=0):
    """Device draw pipeline for blocks blk0..blk0+n-1 of chain's stream (see demcz.h)."""
    L = _lib.load()
    words = np.zeros(2 * n, dtype=np.uint64)
    normals = np.zeros(2 * n)
    logu = np.zeros(n)
    rc = L.demcz_selftest_draws(int(device_id), int(seed), int(chain), int(blk0), int(n),
                                words.ctypes.data_as(C.POINTER(C.c_uint64)), _lib.ptr(normals), _lib.ptr(logu))
    if rc != 0:
        raise DemczError(rc, (L.demcz_last_error(None) or b"").decode())
    return words.reshape(n, 2), normals.reshape(n, 2), logu
