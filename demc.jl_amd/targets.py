"""Device-evaluated log-densities.

The reference takes an arbitrary Julia closure ``logobj(x)::Float64`` (src/demcz.jl:189).  The
three closures its tests and examples build are available as device targets, evaluated inside
the chain-update kernel; any other log-density can be written as a small HIP C++ function
(``ProgramTarget``), which the library compiles at run time into the same kernel; a Python
callable is driven through the host-closure mode (``demcz_propose`` / ``demcz_accept_commit``),
one batch of N proposals per round trip.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass
class MvNormalTarget:
    """``logpdf(MvNormal(mu, Sigma), x)`` -- test/example_normpdf.jl:13-16, README.md:27-28.

    Evaluated as ``c0 - 0.5 * ||W (x - mu)||^2`` with ``W = inv(chol(Sigma))`` (lower
    triangular) and ``c0 = -0.5 (d log 2pi + logdet Sigma)``; ``W`` and ``c0`` are computed
    here once, in float64, and are inputs to the device.
    """
    mu: np.ndarray
    Sigma: np.ndarray

    def __post_init__(self):
        self.mu = np.ascontiguousarray(self.mu, dtype=np.float64)
        self.Sigma = np.ascontiguousarray(self.Sigma, dtype=np.float64)
        d = self.mu.shape[0]
        if self.Sigma.shape != (d, d):
            raise ValueError("Sigma must be d x d")
        L = np.linalg.cholesky(self.Sigma)
        # forward substitution L W = I, row by row (W is lower triangular)
        W = np.zeros((d, d))
        for j in range(d):
            for i in range(j, d):
                s = (1.0 if i == j else 0.0) - float(np.dot(L[i, j:i], W[j:i, j]))
                W[i, j] = s / L[i, i]
        self.W = np.asfortranarray(W)
        self.c0 = -0.5 * (d * math.log(2.0 * math.pi) + 2.0 * float(np.sum(np.log(np.diag(L)))))
        self.d = d

    kind = _lib.TARGET_MVNORMAL

    def fill(self, cfg, keep):
        keep += [self.mu, self.W]
        cfg.mu, cfg.W, cfg.c0 = _lib.ptr(self.mu), _lib.ptr(self.W), self.c0

    def spec(self):
        return dict(kind="mvnormal", mu=self.mu, W=self.W, c0=self.c0)


@dataclass
class IsoQuadTarget:
    """``-sum((x .- mu).^2)`` -- test/test_anneal.jl:10."""
    mu: np.ndarray

    def __post_init__(self):
        self.mu = np.ascontiguousarray(self.mu, dtype=np.float64)
        self.d = self.mu.shape[0]

    kind = _lib.TARGET_ISO_QUAD

    def fill(self, cfg, keep):
        keep += [self.mu]
        cfg.mu = _lib.ptr(self.mu)

    def spec(self):
        return dict(kind="iso_quad", mu=self.mu)


@dataclass
class LinRegSSETarget:
    """``-0.5 * sum((y .- X*b).^2)`` -- test/example_linreg.jl:32.  ``design`` is nobs x d."""
    design: np.ndarray
    y: np.ndarray

    def __post_init__(self):
        self.design = np.asfortranarray(self.design, dtype=np.float64)
        self.y = np.ascontiguousarray(self.y, dtype=np.float64)
        if self.design.shape[0] != self.y.shape[0]:
            raise ValueError("design rows != len(y)")
        self.d = self.design.shape[1]

    kind = _lib.TARGET_LINREG_SSE

    def fill(self, cfg, keep):
        keep += [self.design, self.y]
        cfg.design, cfg.yobs, cfg.nobs = _lib.ptr(self.design), _lib.ptr(self.y), self.design.shape[0]

    def spec(self):
        return dict(kind="linreg_sse", design=self.design, y=self.y)


class _Program:
    """What the program classes share: the normalised ``source`` / ``d`` / ``data`` / ``options``, the arguments as the C ABI takes
    them, and the compile-only check."""

    def _set_program(self, source, d, data, options):
        self.source = str(source)
        self.d = int(d)
        self.data = None if data is None else np.ascontiguousarray(np.ravel(data), dtype=np.float64)
        self.options = (options,) if isinstance(options, str) else tuple(str(o) for o in options)

    def _args(self):
        """(source, options, data pointer or None, ndata) as the C ABI takes them; the data array is kept alive by self."""
        n = 0 if self.data is None else self.data.size
        return self.source.encode(), " ".join(self.options).encode(), (_lib.ptr(self.data) if n else None), n

    def _check(self, name, *mid, tail=()):
        """Call the library's ``name(d, *mid, source, options, *tail)``; raises ``DemczError`` with the last error if it refuses."""
        L = _lib.load()
        src, opts = _Program._args(self)[:2]
        rc = getattr(L, name)(self.d, *mid, src, opts, *tail)
        if rc != 0:
            raise _lib.DemczError(rc, (L.demcz_last_error(None) or b"").decode())


class ProgramTarget(_Program):
    """A log-density written as HIP C++ and compiled for the device at run time (``demcz_set_program``, include/demcz.h).

    ``source`` defines ``__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)``: ``x`` holds the
    ``DEMCZ_D`` (= ``d``) values of the proposal, ``data`` the ``ndata`` doubles of ``data`` (device memory, read-only).  The
    program is compiled with ``--offload-arch=gfx950 -O3 -ffp-contract=off`` followed by ``options`` (e.g. ``["-DNOBS=40"]``):
    a fused multiply-add happens only where ``fma()`` is written.  ``d`` must be in 1..32.

    With ``lanes_per_chain=demc.LAYOUT_PROGRAM_WAVE`` (``HipEngine``, ``demcz_sample``, ``demcz_anneal``) the same program runs on
    the wave-per-chain layout (N <= 2048; measured at N = 1024: 4.6-11.7 x less kernel time); same results bit for bit.  The function is then called for all 31
    candidates of a five-generation pass, most of them never taken: it must be a pure function of (x, data) that terminates for
    every finite x.
    """
    kind = _lib.TARGET_PROGRAM

    def __init__(self, source: str, d: int, data=None, options=()):
        self._set_program(source, d, data, options)

    def _args(self):
        return super()._args()[:2]

    def check(self, layout=None):
        """Compile the program (no device needed); raises ``DemczError`` with the compiler log if it does not compile.
        ``layout``: the ``lanes_per_chain`` the handle will be created with -- ``demc.LAYOUT_PROGRAM_WAVE`` compiles the unit of the
        wave-per-chain layout (d in 2..32), where a program that needs many registers or does not inline shows it; None, 0 or 1 the
        one-lane unit."""
        if layout is None:
            self._check("demcz_program_check")
        else:
            self._check("demcz_program_check_layout", tail=(int(layout),))

    def check_bridge(self):
        """Compile the program's bridge-sampling unit (``demcz_bridge_check``; no device needed): what ``HipEngine.bridge`` and
        ``demc.bridge_chain`` compile on first use.  Raises ``DemczError`` with the compiler log if it does not compile."""
        self._check("demcz_bridge_check")

    def fill(self, cfg, keep):
        pass                # (the program and its data go to the handle after demcz_create: attach)

    def attach(self, L, h):
        """``demcz_set_program`` on a freshly created handle; returns the status."""
        return L.demcz_set_program(h, *super()._args())


class DerivedProgram(_Program):
    """``m`` functions of every draw, written as HIP C++ and run on the device over a history (``demcz_derive``, include/demcz.h):
    what Stan calls generated quantities.

    ``source`` defines ``__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata,
    double* out)``: ``x`` holds the ``DEMCZ_D`` (= ``d``) parameters of one draw, ``logp`` its ``log_obj`` (NaN where the source
    keeps none), ``data`` the ``ndata`` doubles of ``data`` (device memory, read-only, NULL without data), ``out`` the
    ``DEMCZ_M`` (= ``m``) results, preset to NaN.  Compiled like a ``ProgramTarget``: ``-O3 -ffp-contract=off`` followed by
    ``options``.  ``d`` and ``m`` must be in 1..32; ``names`` optionally labels the ``m`` results.

    The function is called once per draw in no particular order, so it must be a pure function of its arguments.
    Runtime-indexed ``x[j]`` or ``out[k]`` inside the function sends those arrays to scratch memory; loops over the compile-time
    ``DEMCZ_D`` and ``DEMCZ_M`` unroll and avoid that.

    Used through ``HipEngine.derive``, ``demc.derive_chain`` or a runner's ``derive``; each returns a ``DerivedHistory``.
    """

    def __init__(self, source: str, d: int, m: int, data=None, options=(), names=None):
        self._set_program(source, d, data, options)
        self.m = int(m)
        self.names = None if names is None else [str(n) for n in names]
        if self.names is not None and len(self.names) != self.m:
            raise ValueError("names must hold m labels")

    def check(self):
        """Compile the program (no device needed); raises ``DemczError`` with the compiler log if it does not compile."""
        self._check("demcz_derive_check", self.m)


class PredictiveProgram(DerivedProgram):
    """A ``DerivedProgram`` that is also given random numbers (``demcz_predict`` and ``demcz_ppc``, include/demcz.h): replicated
    data ``y_rep ~ p(y | theta)``, predictive draws at new covariates, posterior predictive p-values.

    ``source`` defines ``__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata,
    demcz_rng* rng, double* out)``; everything but ``rng`` is ``DerivedProgram``'s, limits and compile options included.  ``rng``
    is the draw's own stream, consumed through ``demcz_uniform(rng)`` (in (0, 1)), ``demcz_normal(rng)``,
    ``demcz_exponential(rng)`` and ``demcz_bits(rng, &r1, &r2)`` (128 raw bits).  The stream of the draw of global chain ``c`` at
    generation ``g`` is keyed by ``(seed, g, c)`` and by nothing else: the numbers do not depend on the
    window asked for, the launch, the sharding or ``set_history_origin``, and a draw may take as many as it likes.

    Two programs run with one seed are given the same random numbers: pass different seeds where their results must be
    independent.

    Used through ``HipEngine.predict`` and ``HipEngine.ppc`` (also on a ``DerivedHistory``), ``demc.predict_chain`` and
    ``demc.ppc_chain``.
    """

    def check(self):
        """Compile the program (no device needed); raises ``DemczError`` with the compiler log if it does not compile."""
        self._check("demcz_predict_check", self.m)


class PointwiseProgram(_Program):
    """The log-likelihood of every observation at a draw, written as HIP C++ and run on the device over a history
    (``demcz_pointwise`` and ``demcz_loo``, include/demcz.h): the input of PSIS-LOO and WAIC.

    ``source`` defines ``__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)``: ``x``
    holds the ``DEMCZ_D`` (= ``d``) parameters of one draw, ``data`` the ``ndata`` doubles of ``data`` (device memory,
    read-only, NULL without data), ``i`` the observation, ``0 <= i < nobs``.  Compiled like a ``DerivedProgram``:
    ``-O3 -ffp-contract=off`` followed by ``options``.  ``d`` must be in 1..32; ``names`` optionally labels the observations.

    It must be a pure function of its arguments.  A lane keeps its draw in registers while it walks the observations; indexing
    ``x`` with a run-time value sends it to scratch memory, loops over the compile-time ``DEMCZ_D`` unroll and avoid that.

    Used through ``HipEngine.pointwise`` and ``HipEngine.loo``, ``demc.pointwise_chain`` and ``demc.loo_chain``.
    """

    def __init__(self, source: str, d: int, nobs: int, data=None, options=(), names=None):
        self._set_program(source, d, data, options)
        self.nobs = int(nobs)
        if self.nobs < 1:
            raise ValueError("nobs must be at least 1")
        self.names = None if names is None else [str(n) for n in names]
        if self.names is not None and len(self.names) != self.nobs:
            raise ValueError("names must hold nobs labels")

    def check(self):
        """Compile the program (no device needed); raises ``DemczError`` with the compiler log if it does not compile."""
        self._check("demcz_pointwise_check")


def is_device_target(obj) -> bool:
    return isinstance(obj, (MvNormalTarget, IsoQuadTarget, LinRegSSETarget, ProgramTarget))
