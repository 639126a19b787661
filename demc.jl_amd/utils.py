"""Post-hoc diagnostics with the reference's names (src/utils.jl), reduced on the GPU.

``Rhat_gelman``, ``mean_cov_chain`` and ``convergence_check`` take the host arrays the reference's
examples pass them (test/example_normpdf.jl:35-47); the arrays are uploaded and reduced by the same
kernels the autostop uses.  ``flatten_chain`` is a pure re-indexing (utils.jl:22-32).  ``extract_best``
(utils.jl:120-125) finds the best draw on the device.  Plotting and ``save_res`` are not reproduced (dead code in Julia >= 1.0,
SURVEY.md Q16).
Beyond the reference: ``ess_chain``, ``autocov_chain``, ``quantile_chain`` and ``posterior_summary`` (effective sample size and
quantiles by exact selection), ``derive_chain`` (functions of the draws, evaluated on the device), and
``rank_normalize_chain`` / ``rank_diagnostics_chain`` (exact ranks on the device: rank-normalised R-hat, bulk- and tail-ESS),
``histogram_chain`` / ``histogram2d_chain`` / ``hdi_chain`` (the counts behind a marginal density and a corner plot, and the
highest-density interval; the drawing itself stays out of scope).
Checkpoints: the reference only resumes in memory (``prevrun=``); ``save_checkpoint`` /
``load_checkpoint`` put the same information in one ``.npz`` file.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DemczError
from .sampler import MC


def _chk(rc):
    if rc != 0:
        raise DemczError(rc, (_lib.load().demcz_last_error(None) or b"").decode())


def Rhat_gelman(chain, Npop=None, Ngeneration=None, Npar=None, device_id=0):
    """Split-chain Gelman-Rubin statistic per parameter, src/utils.jl:2-20."""
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    if (Npop, Ngeneration, Npar) != (None, None, None):
        assert (Npop or N, Npar or d) == (N, d) and (Ngeneration or G) <= G
        G = Ngeneration or G
        chain = _lib.f64(chain[:, :, :G], "F")
    out = np.empty(d)
    _chk(_lib.load().demcz_rhat_array(device_id, _lib.ptr(chain), N, d, G, _lib.ptr(out)))
    return out


def flatten_chain(chain, Npop=None, Ngeneration=None, Npar=None):
    """Npar x (Npop*Ngeneration) matrix, generation-major then chain, src/utils.jl:22-32."""
    chain = np.asarray(chain)
    N, d, G = chain.shape
    return chain.transpose(1, 2, 0).reshape(d, G * N)


def accept_ratio(log_obj, device_id=0):
    """sum(diff(log_obj, dims=2) .!= 0, dims=2) ./ (Ngeneration-1), src/utils.jl:61."""
    log_obj = _lib.f64(log_obj, "F")
    N, G = log_obj.shape
    out = np.empty(N)
    _chk(_lib.load().demcz_accept_ratio_array(device_id, _lib.ptr(log_obj), N, G, _lib.ptr(out)))
    return out


def mean_cov_chain(chain, Npop=None, Ngeneration=None, Npar=None, device_id=0):
    """Mean over all Npop*Ngeneration draws and their 1/(Npop*Ngeneration) covariance, src/utils.jl:96-111."""
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    mean = np.empty(d)
    cov = np.empty((d, d), order="F")
    _chk(_lib.load().demcz_mean_cov_array(device_id, _lib.ptr(chain), N, d, G, _lib.ptr(mean), _lib.ptr(cov)))
    return mean, cov


def ess_chain(chain, max_lag=0, device_id=0):
    """Effective sample size per parameter of an Npop x Npar x Ngeneration history (BDA3 section 11.5 / Stan, on the split chains
    of Rhat_gelman, on the values as they are; rank_diagnostics_chain has the rank-normalised bulk and tail ESS): an ESS tuple (ess, tau, varplus, pairs, converged).  Not in the reference."""
    from .engine import ESS
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    out = ESS(np.empty(d), np.empty(d), np.empty(d), np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int32))
    _chk(_lib.load().demcz_ess_array(device_id, _lib.ptr(chain), N, d, G, int(max_lag), _lib.ptr(out.ess), _lib.ptr(out.tau),
                                     _lib.ptr(out.varplus), _lib.ptr(out.pairs, _lib._lp), _lib.ptr(out.converged, _lib._ip)))
    return out


def autocov_sums_chain(chain, lag_from, lag_to, device_id=0):
    """d x (lag_to - lag_from + 1): sum over the 2 Npop split chains of n c_j(t) (demcz_autocov_sums_array)."""
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    out = np.empty((d, max(0, int(lag_to) - int(lag_from) + 1)), order="F")
    _chk(_lib.load().demcz_autocov_sums_array(device_id, _lib.ptr(chain), N, d, G, int(lag_from), int(lag_to), _lib.ptr(out)))
    return out


def autocov_chain(chain, max_lag, device_id=0):
    """A(t) = mean over the split chains of their biased autocovariance c_j(t), t = 0 .. L: Npar x (L + 1), with L = n - 1 for
    max_lag <= 0 and min(n - 1, max_lag) otherwise, n = Ngeneration // 2."""
    N, _, G = np.shape(chain)
    n = G // 2
    L = n - 1 if max_lag <= 0 else min(n - 1, int(max_lag))
    return autocov_sums_chain(chain, 0, L, device_id) / (2.0 * N * n)


def quantile_chain(chain, probs, device_id=0, with_order_stats=False):
    """Quantiles per parameter of an Npop x Npar x Ngeneration history over all its draws: Npar x len(probs), Hyndman-Fan type 7
    (np.quantile's default) between two order statistics found exactly by a radix select on the device (demcz_quantiles_array).
    `with_order_stats`: a Quantiles tuple (q, lower, upper).  A parameter that holds a NaN is NaN.  Not in the reference."""
    from .engine import Quantiles
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    probs = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    nq = probs.size
    out = Quantiles(np.empty((d, nq), order="F"), np.empty((d, nq), order="F"), np.empty((d, nq), order="F"))
    _chk(_lib.load().demcz_quantiles_array(device_id, _lib.ptr(chain), N, d, G, nq, _lib.ptr(probs), _lib.ptr(out.q),
                                           _lib.ptr(out.lower), _lib.ptr(out.upper)))
    return out if with_order_stats else out.q


def best_logobj(log_obj, device_id=0):
    """(bestval, chain, column), 0-based: the maximum of an Npop x Ngeneration log_obj ignoring NaN, ties (by ==) to the earliest
    generation and then to the lowest chain, as findn(bestval .== log_obj) lists them (demcz_best_array).  All NaN: (nan, -1, -1)."""
    log_obj = _lib.f64(log_obj, "F")
    N, G = log_obj.shape
    v, c, g = C.c_double(), C.c_int64(), C.c_int64()
    _chk(_lib.load().demcz_best_array(device_id, _lib.ptr(log_obj), N, G, C.byref(v), C.byref(c), C.byref(g)))
    return v.value, c.value, g.value


def extract_best(mc, device_id=0):
    """(bestval, bestpar) of a run, src/utils.jl:120-125: the largest log_obj and the parameters that gave it."""
    bestval, c, g = best_logobj(mc.log_obj, device_id)
    if c < 0:
        return bestval, np.full(np.shape(mc.chain)[1], np.nan)
    return bestval, np.array(mc.chain[c, :, g])


def rank_normalize_chain(chain, center=None, ranks=False, device_id=0):
    """The normal scores of the exact average ranks of every draw of an Npop x Npar x Ngeneration history among all draws of its
    parameter -- a ``DerivedHistory`` on the device, generations 1..Ngeneration (demcz_rank_normalize_array).  ``center`` (Npar
    values): rank ``fabs(x - center)``; ``ranks``: the average ranks themselves.  Not in the reference."""
    from .engine import DerivedHistory
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    ctr = None
    if center is not None:
        ctr = _lib.f64(center)
        if ctr.shape != (d,):
            raise ValueError("center must have Npar entries")
    L = _lib.load()
    out = C.c_void_p()
    _chk(L.demcz_rank_normalize_array(device_id, _lib.ptr(chain), N, d, G, 1 if ranks else 0, _lib.ptr(ctr), C.byref(out)))
    return DerivedHistory(L, out, N, d, 1, G)


def rank_diagnostics_chain(chain, device_id=0):
    """RankDiagnostics(rhat_rank, ess_bulk, ess_tail) per parameter of an Npop x Npar x Ngeneration history (Vehtari et al. 2021;
    demcz_rank_diagnostics_array).  Not in the reference."""
    from .engine import RankDiagnostics
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    out = RankDiagnostics(np.empty(d), np.empty(d), np.empty(d))
    _chk(_lib.load().demcz_rank_diagnostics_array(device_id, _lib.ptr(chain), N, d, G, _lib.ptr(out.rhat_rank), _lib.ptr(out.ess_bulk),
                                                  _lib.ptr(out.ess_tail)))
    return out


def histogram_chain(chain, bins=33, range=None, device_id=0):
    """Marginal histograms of every parameter of an Npop x Npar x Ngeneration history over all its draws (demcz_histogram_array): a
    ``Histogram`` with np.histogram's counts.  ``range``: (lo, hi), Npar x 2, or None (the smallest and largest draw of each
    parameter).  Not in the reference beyond the 33-bin histogram its convergence_check once drew."""
    from .engine import Histogram, _range_args
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    nb = int(bins)
    lo, hi = _range_args(range, d)
    out = Histogram(np.zeros((d, max(nb, 0)), dtype=np.int64), np.empty((d, max(nb, 0) + 1)), np.zeros(d, dtype=np.int64),
                    np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int64))
    _chk(_lib.load().demcz_histogram_array(device_id, _lib.ptr(chain), N, d, G, nb, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(out.edges),
                                           _lib.ptr(out.counts, _lib._lp), _lib.ptr(out.below, _lib._lp), _lib.ptr(out.above, _lib._lp),
                                           _lib.ptr(out.nan, _lib._lp)))
    return out


def histogram2d_chain(chain, pairs=None, bins=32, range=None, device_id=0):
    """Pairwise histograms of an Npop x Npar x Ngeneration history (demcz_histogram2d_array): a ``Histogram2D`` with
    np.histogram2d's counts for every pair (default: all p < q).  ``bins``: one number or (nbx, nby), each 1 to 128."""
    from .engine import Histogram2D, _bins2, _pairs_arg, _range_args
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    nbx, nby = _bins2(bins)
    pr = _pairs_arg(pairs, d)
    lo, hi = _range_args(range, d)
    npairs = pr.shape[0]
    counts = np.zeros((npairs, max(nbx, 0), max(nby, 0)), dtype=np.int64)
    ex, ey = np.empty((d, max(nbx, 0) + 1)), np.empty((d, max(nby, 0) + 1))
    outside = np.zeros(npairs, dtype=np.int64)
    _chk(_lib.load().demcz_histogram2d_array(device_id, _lib.ptr(chain), N, d, G, npairs, _lib.ptr(pr, _lib._ip), nbx, nby, _lib.ptr(lo),
                                             _lib.ptr(hi), _lib.ptr(ex), _lib.ptr(ey), _lib.ptr(counts, _lib._lp),
                                             _lib.ptr(outside, _lib._lp)))
    return Histogram2D(counts, pr, (ex, ey), outside)


def hdi_chain(chain, prob=0.94, device_id=0):
    """The highest-density interval of every parameter of an Npop x Npar x Ngeneration history (demcz_hdi_array; ArviZ's unimodal
    hdi): Npar x 2, or Npar x nprob x 2 for several probabilities.  A parameter that holds a NaN is NaN."""
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    probs = np.ascontiguousarray(np.atleast_1d(prob), dtype=np.float64)
    out = np.empty((d, probs.size, 2))
    _chk(_lib.load().demcz_hdi_array(device_id, _lib.ptr(chain), N, d, G, probs.size, _lib.ptr(probs), _lib.ptr(out)))
    return out[:, 0, :] if np.ndim(prob) == 0 else out


def posterior_summary(chain, device_id=0, probs=None, rank_normalized=False, hdi_prob=None):
    """Per parameter: mean, sd = sqrt(var+), mcse = sqrt(var+ / ess), ess, rhat, converged (of the ESS: 0 where the lags ran out
    and ess is an upper bound) -- mean_cov_chain, Rhat_gelman and ess_chain, all reduced on the device.  With `probs`, also
    quantiles = quantile_chain(chain, probs): Npar x len(probs).  With `rank_normalized`, also rhat_rank, ess_bulk and ess_tail
    (rank_diagnostics_chain).  With `hdi_prob`, also hdi = hdi_chain(chain, hdi_prob)."""
    mean, _ = mean_cov_chain(chain, device_id=device_id)
    e = ess_chain(chain, device_id=device_id)
    with np.errstate(all="ignore"):
        out = dict(mean=mean, sd=np.sqrt(e.varplus), mcse=np.sqrt(e.varplus / e.ess), ess=e.ess,
                   rhat=Rhat_gelman(chain, device_id=device_id), converged=e.converged)
    if probs is not None:
        out["quantiles"] = quantile_chain(chain, probs, device_id=device_id)
    if rank_normalized:
        out.update(rank_diagnostics_chain(chain, device_id=device_id)._asdict())
    if hdi_prob is not None:
        out["hdi"] = hdi_chain(chain, hdi_prob, device_id=device_id)
    return out


def _program_arrays(chain, log_obj, program):
    """The column-major arrays of a history as the _array entry points of a per-draw program take them, checked against it."""
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    if program.d != d:
        raise ValueError("the program's d is not the chain's Npar")
    lo = None
    if log_obj is not None:
        lo = _lib.f64(log_obj, "F")
        if lo.shape != (N, G):
            raise ValueError("log_obj must be Npop x Ngeneration")
    return chain, lo, N, d, G


def derive_chain(chain, log_obj, program, device_id=0):
    """``program`` (a ``DerivedProgram``) evaluated on every draw of an Npop x Npar x Ngeneration history and its
    Npop x Ngeneration ``log_obj`` (or None: the program's ``logp`` is NaN) -- a ``DerivedHistory`` on the device, generations
    1..Ngeneration (demcz_derive_array).  The uploaded arrays are not kept.  Not in the reference."""
    from .engine import DerivedHistory
    chain, lo, N, d, G = _program_arrays(chain, log_obj, program)
    src, opts, data, ndata = program._args()
    L = _lib.load()
    out = C.c_void_p()
    _chk(L.demcz_derive_array(device_id, _lib.ptr(chain), _lib.ptr(lo), N, d, G, program.m, src, opts, data, ndata, C.byref(out)))
    return DerivedHistory(L, out, N, program.m, 1, G, program.names)


def predict_chain(chain, log_obj, program, seed, chain_id0=0, device_id=0):
    """``program`` (a ``PredictiveProgram``) at every draw of an Npop x Npar x Ngeneration history (``log_obj`` or None as for
    ``derive_chain``), the draw of row ``i`` at generation ``g`` with the random stream of (seed, g, chain_id0 + i) -- a
    ``DerivedHistory`` on the device, generations 1..Ngeneration (demcz_predict_array).  Not in the reference."""
    from .engine import DerivedHistory
    chain, lo, N, d, G = _program_arrays(chain, log_obj, program)
    src, opts, data, ndata = program._args()
    L = _lib.load()
    out = C.c_void_p()
    _chk(L.demcz_predict_array(device_id, _lib.ptr(chain), _lib.ptr(lo), N, d, G, program.m, src, opts, data, ndata,
                               int(seed) & (2**64 - 1), int(chain_id0), C.byref(out)))
    return DerivedHistory(L, out, N, program.m, 1, G, program.names, int(chain_id0))


def ppc_chain(chain, log_obj, program, seed, chain_id0=0, observed=None, device_id=0):
    """The posterior predictive check of ``program`` over such a history (demcz_ppc_array): a ``PPC`` record of the counts of its m
    columns against ``observed`` (m values; None: zeros), of the values ``predict_chain`` would have written.  Not in the reference."""
    from .engine import _ppc_observed, ppc_record
    chain, lo, N, d, G = _program_arrays(chain, log_obj, program)
    obs = _ppc_observed(observed, program.m)
    src, opts, data, ndata = program._args()
    counts = np.zeros(3 * program.m, dtype=np.int64)
    _chk(_lib.load().demcz_ppc_array(device_id, _lib.ptr(chain), _lib.ptr(lo), N, d, G, program.m, src, opts, data, ndata,
                                     int(seed) & (2**64 - 1), int(chain_id0), _lib.ptr(obs), _lib.ptr(counts, _lib._lp)))
    return ppc_record(counts, N * G, program.names)


def pointwise_chain(chain, program, obs_from=0, obs_to=None, device_id=0):
    """The log-likelihoods of observations obs_from .. obs_to - 1 (at most 32) of ``program`` (a ``PointwiseProgram``) at every
    draw of an Npop x Npar x Ngeneration history -- a ``DerivedHistory`` on the device, generations 1..Ngeneration
    (demcz_pointwise_array).  Not in the reference."""
    from .engine import DerivedHistory
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    if program.d != d:
        raise ValueError("the program's d is not the chain's Npar")
    obs_from = int(obs_from)
    obs_to = program.nobs if obs_to is None else int(obs_to)
    if not 0 <= obs_from < obs_to <= program.nobs:
        raise ValueError("need 0 <= obs_from < obs_to <= nobs")
    src, opts, data, ndata = program._args()
    L = _lib.load()
    out = C.c_void_p()
    _chk(L.demcz_pointwise_array(device_id, _lib.ptr(chain), N, d, G, obs_from, obs_to - obs_from, src, opts, data, ndata, C.byref(out)))
    names = None if program.names is None else program.names[obs_from:obs_to]
    return DerivedHistory(L, out, N, obs_to - obs_from, 1, G, names)


def loo_columns_chain(loglik, r_eff=None, names=None, device_id=0):
    """PSIS-LOO and WAIC of an Npop x nobs x Ngeneration array of pointwise log-likelihoods computed elsewhere
    (demcz_loo_columns_array): a ``LOO`` record.  ``r_eff``: a value or nobs values in (0, inf).  Not in the reference."""
    from .engine import loo_record, _loo_outputs, _r_eff_arg
    loglik = _lib.f64(loglik, "F")
    N, nobs, G = loglik.shape
    e, k, n, l, w = _loo_outputs(nobs)
    r = _r_eff_arg(r_eff, nobs)
    _chk(_lib.load().demcz_loo_columns_array(device_id, _lib.ptr(loglik), N, nobs, G, _lib.ptr(r), _lib.ptr(e), _lib.ptr(k),
                                             _lib.ptr(n, _lib._lp), _lib.ptr(l), _lib.ptr(w)))
    return loo_record(e, k, n, l, w, N * G, names)


def loo_chain(chain, program, r_eff=None, device_id=0):
    """PSIS-LOO and WAIC of ``program`` (a ``PointwiseProgram``) over every draw of an Npop x Npar x Ngeneration history
    (demcz_loo_array): a ``LOO`` record.  Not in the reference."""
    from .engine import loo_record, _loo_outputs, _r_eff_arg
    chain = _lib.f64(chain, "F")
    N, d, G = chain.shape
    if program.d != d:
        raise ValueError("the program's d is not the chain's Npar")
    nobs = program.nobs
    e, k, n, l, w = _loo_outputs(nobs)
    r = _r_eff_arg(r_eff, nobs)
    src, opts, data, ndata = program._args()
    _chk(_lib.load().demcz_loo_array(device_id, _lib.ptr(chain), N, d, G, nobs, src, opts, data, ndata, _lib.ptr(r), _lib.ptr(e),
                                     _lib.ptr(k), _lib.ptr(n, _lib._lp), _lib.ptr(l), _lib.ptr(w)))
    return loo_record(e, k, n, l, w, N * G, program.names)


def _program_args(program):
    src, opts = program._args()
    n = 0 if program.data is None else program.data.size
    return src, opts, (_lib.ptr(program.data) if n else None), n


def bridge_chain(chain, log_obj, program, seed=0x9E3779B97F4A7C15, neff=None, tol=1e-10, max_iter=1000, device_id=0):
    """The marginal likelihood by bridge sampling of an Npop x Npar x Ngeneration history and its Npop x Ngeneration log_obj, the
    target given as a ``ProgramTarget`` (demcz_bridge_array): a ``Bridge`` record.  The whole history is the window: its first
    half fits the proposal.  ``neff``: the effective number of posterior draws of the second half (None: all of them);
    ``seed``: the proposal's streams, not the run's own seed.  Not in the reference."""
    from .engine import _bridge_outputs, _bridge_out_args, _bridge_record
    chain = _lib.f64(chain, "F")
    log_obj = _lib.f64(log_obj, "F")
    N, d, G = chain.shape
    if log_obj.shape != (N, G):
        raise ValueError("log_obj must be Npop x Ngeneration")
    if program.d != d:
        raise ValueError("the program's d is not the chain's Npar")
    src, opts, data, ndata = _program_args(program)
    o = _bridge_outputs(d)
    _chk(_lib.load().demcz_bridge_array(device_id, _lib.ptr(chain), _lib.ptr(log_obj), N, d, G, src, opts, data, ndata,
                                        int(seed) & (2**64 - 1), 0.0 if neff is None else float(neff), float(tol), int(max_iter),
                                        *_bridge_out_args(o)))
    return _bridge_record(o)


def bridge_posterior_chain(chain, log_obj, mean, L, device_id=0):
    """a1 = log_obj - log g(x), g = N(mean, L L^T), of every draw of an Npop x Npar x Ngeneration history
    (demcz_bridge_posterior_array): a one-column ``DerivedHistory`` on the device, generations 1..Ngeneration."""
    from .engine import DerivedHistory, _bridge_ml
    chain = _lib.f64(chain, "F")
    log_obj = _lib.f64(log_obj, "F")
    N, d, G = chain.shape
    if log_obj.shape != (N, G):
        raise ValueError("log_obj must be Npop x Ngeneration")
    mean, L = _bridge_ml(mean, L, d)
    lib = _lib.load()
    out = C.c_void_p()
    _chk(lib.demcz_bridge_posterior_array(device_id, _lib.ptr(chain), _lib.ptr(log_obj), N, d, G, _lib.ptr(mean), _lib.ptr(L), C.byref(out)))
    return DerivedHistory(lib, out, N, 1, 1, G, ["a1"])


def bridge_proposal_program(program, Np, wp, mean, L, seed, want_draws=False, device_id=0):
    """Np x wp fresh draws of g = N(mean, L L^T) and a2 = logobj(x) - log g(x) of a ``ProgramTarget`` without an engine
    (demcz_bridge_proposal_program): a one-column ``DerivedHistory``, or with ``want_draws`` the pair (a2, draws)."""
    from .engine import DerivedHistory, _bridge_ml
    mean, L = _bridge_ml(mean, L, program.d)
    src, opts, data, ndata = _program_args(program)
    lib = _lib.load()
    a2, xs = C.c_void_p(), C.c_void_p()
    _chk(lib.demcz_bridge_proposal_program(device_id, program.d, int(Np), int(wp), int(seed) & (2**64 - 1), _lib.ptr(mean), _lib.ptr(L),
                                           src, opts, data, ndata, C.byref(a2), C.byref(xs) if want_draws else None))
    ha = DerivedHistory(lib, a2, int(Np), 1, 1, int(wp), ["a2"])
    return (ha, DerivedHistory(lib, xs, int(Np), program.d, 1, int(wp))) if want_draws else ha


def convergence_check(chain, log_obj, figure_path=None, verbose=True, parnames=None, device_id=0):
    """(accept_ratio, Rhat) as src/utils.jl:34-94 returns them (the plotting part is commented out
    in the reference and is not reproduced)."""
    chain = np.asarray(chain)
    log_obj = np.asarray(log_obj)
    Npop, Npar, Ngeneration = chain.shape
    if log_obj.shape != (Npop, Ngeneration):
        raise ValueError("log_obj must be Npop x Ngeneration")                         # utils.jl:40-46
    acc = accept_ratio(log_obj, device_id)
    Rhat = Rhat_gelman(chain, device_id=device_id)
    if verbose:
        print("Summary Checks\n\nAcceptance Ratio of each chain:")
        print(acc)
        print(f"\nRhat Gelman: {Rhat}\n")
    return acc, Rhat


_NO_SEED = object()


def save_checkpoint(path, mc: MC, Z, generations_done=None, seed=_NO_SEED, opts=None):
    """Everything a resumed run needs: final states, archive, how far the RNG streams have advanced
    (`generations_done`; default: what `mc` itself records, MC.generations_drawn) and the `seed` of the run -- REQUIRED
    (positionally or by keyword): a checkpoint written with a wrong seed resumes on another Philox stream, silently."""
    if seed is _NO_SEED:
        raise TypeError("save_checkpoint: pass the run's seed (the one given to demcz_sample / demcz_anneal)")
    if generations_done is None:
        generations_done = mc.generations_drawn
    np.savez_compressed(path, Xcurrent=mc.Xcurrent, log_objcurrent=mc.log_objcurrent, last_chain=mc.chain[:, :, -1:],
                        last_log_obj=mc.log_obj[:, -1:], Z=Z, generations_done=int(generations_done), seed=int(seed),
                        blocks_per_generation=int(getattr(mc, "rng_blocks_per_generation", None) or 0))


def load_checkpoint(path):
    """Returns (prevrun, Z, generations_done, seed): pass ``prevrun=prevrun, seed=seed`` to ``demcz_sample`` to continue
    the same streams -- the returned ``prevrun`` keeps only the last generation of the history but records
    ``generations_done`` (MC.rng_generations), so the resumed run draws what an uninterrupted one would."""
    f = np.load(path)
    prev = MC(np.asfortranarray(f["last_chain"]), np.asfortranarray(f["last_log_obj"]), np.asfortranarray(f["Xcurrent"]),
              np.array(f["log_objcurrent"]), rng_generations=int(f["generations_done"]),
              rng_blocks_per_generation=(int(f["blocks_per_generation"]) or None) if "blocks_per_generation" in f else None)
    return prev, np.asfortranarray(f["Z"]), int(f["generations_done"]), int(f["seed"])
