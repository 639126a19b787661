"""Extended-precision reference of the post-hoc statistics, src/utils.jl:2-20 (split R-hat), :61 (accept ratio) and :96-111 (mean and
covariance), for the tests of the device statistics (test_stats_reference.py proves it against exact rational arithmetic,
test_gpu_stats.py holds the kernels to it).

The oracle's own statistics are float64 loops: on data whose mean is 1e6 standard deviations from zero they carry errors of the
size the device tolerances allow, so they cannot judge the device.  Here every formula is evaluated two-pass (means first, then
sums of squared deviations) in numpy.longdouble (64-bit significand, eps 1.1e-19), or, on a platform whose long double is no wider
than a double, in mpmath at 40 digits.

One step is not in the Julia: the data are centred on the first sample of chain 0 before anything else.  The difference of two
doubles is rounded once in the wide format, an error of 5e-20 of the distance between a sample and the pivot -- which is itself
a sample, so that distance is a few standard deviations, never the offset.  R-hat and the covariance do not depend on a common
shift, and the mean gets the pivot back at the end.  Without it `avg_chains .- avg_par` (utils.jl:13) would subtract two rounded
numbers of size 1e6 and the reference would be good to 1e-13 only (test_stats_reference.py holds it to 1e-17 against fractions).

IEEE semantics: W = 0 gives +inf (B > 0) or nan (B = 0), as Julia's `sqrt.(varhat ./ W)` does.
"""
from fractions import Fraction

import numpy as np

LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 2e-19)
MP_DIGITS = 40


# ---- the two number systems ------------------------------------------------------------------------------------------------------
class _LD:
    """numpy.longdouble arrays."""
    name = "longdouble"

    @staticmethod
    def lift(a):
        return np.asarray(a, dtype=np.longdouble)

    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            return a / b

    @staticmethod
    def sqrt(a):
        with np.errstate(all="ignore"):
            return np.sqrt(a)

    @staticmethod
    def fraction(v):
        v = np.longdouble(v)
        hi = float(v)
        lo = float(v - np.longdouble(hi))                  # (a 64-bit significand is two doubles exactly)
        assert np.longdouble(hi) + np.longdouble(lo) == v
        return Fraction(hi) + Fraction(lo)


class _MP:
    """NumPy object arrays of mpmath.mpf at MP_DIGITS digits (+, -, *, sum and mean go through the elements' own operators)."""
    name = "mpmath"

    @staticmethod
    def _mp():
        import mpmath
        mpmath.mp.dps = MP_DIGITS
        return mpmath

    @classmethod
    def lift(cls, a):
        mp = cls._mp()
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [mp.mpf(float(v)) for v in a.ravel()]
        return out

    @classmethod
    def div(cls, a, b):
        mp = cls._mp()
        a, b = np.broadcast_arrays(np.asarray(a, dtype=object), np.asarray(b, dtype=object))
        out = np.empty(a.shape, dtype=object)
        for i in np.ndindex(a.shape):
            if b[i] != 0:
                out[i] = a[i] / b[i]
            else:
                out[i] = mp.nan if a[i] == 0 or a[i] != a[i] else (mp.inf if a[i] > 0 else -mp.inf)
        return out

    @classmethod
    def sqrt(cls, a):
        mp = cls._mp()
        out = np.empty(np.shape(a), dtype=object)
        for i in np.ndindex(out.shape):
            out[i] = mp.sqrt(a[i]) if a[i] == a[i] and a[i] >= 0 else mp.nan
        return out

    @classmethod
    def fraction(cls, v):
        cls._mp()
        sign, man, exp, _ = v._mpf_
        f = Fraction(int(man)) * (Fraction(2) ** int(exp))
        return -f if sign else f


def backend(name=None):
    """The number system in use: long double where it is wider than a double (checked at import), mpmath otherwise.  `name`
    ("longdouble" / "mpmath") forces one, for the test that the two agree."""
    if name is None:
        return _LD if LONGDOUBLE else _MP
    return {"longdouble": _LD, "mpmath": _MP}[name]


def to_float(a):
    """Round an extended array to float64 (+-inf and nan kept)."""
    a = np.asarray(a)
    if a.dtype != object:
        return np.asarray(a, dtype=np.float64)
    return np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def _centred(B, chain):
    """(chain - pivot, pivot) in B's numbers, pivot[p] = chain[0, p, 0]."""
    x = B.lift(chain)
    pivot = x[:1, :, :1]
    return x - pivot, pivot


def _mean(a, axes):
    """Mean over `axes` (kept): the sum, then one division by the count."""
    cnt = 1
    for ax in axes:
        cnt *= a.shape[ax]
    return a.sum(axis=axes, keepdims=True) / cnt


# ---- src/utils.jl ---------------------------------------------------------------------------------------------------------------
def rhat_parts(chain, use=None):
    """Rhat_gelman, src/utils.jl:2-20, line by line; returns dict(B, W, varhat, rhat2, rhat) of extended arrays of Npar."""
    Bk = backend(use)
    chain = np.asarray(chain, dtype=np.float64)
    Npop, Npar, Ngeneration = chain.shape
    n = Ngeneration // 2                                                    # :4 (an odd window drops its last sample)
    m = Npop * 2                                                            # :5
    if n < 2:
        raise ValueError("split R-hat needs at least 4 generations")
    c, _ = _centred(Bk, chain[:, :, :2 * n])
    cs = np.concatenate([c[:, :, :n], c[:, :, n:2 * n]], axis=0)            # :6-8
    avg_par = _mean(cs, (0, 2))                                             # :10
    avg_chains = _mean(cs, (2,))                                            # :11
    B = (((avg_chains - avg_par) ** 2).sum(axis=0) * n / (m - 1)).ravel()   # :13
    sj = ((cs - avg_chains) ** 2).sum(axis=2, keepdims=True) / (n - 1)      # :14
    W = (sj.sum(axis=0) / m).ravel()                                        # :15
    varhat = W * (n - 1) / n + B / n                                        # :16
    rhat2 = Bk.div(varhat, W)
    return dict(B=B, W=W, varhat=varhat, rhat2=rhat2, rhat=Bk.sqrt(rhat2))   # :18


def rhat_gelman(chain, use=None):
    """Split R-hat per parameter, rounded to float64."""
    return to_float(rhat_parts(chain, use)["rhat"])


def mean_cov_ext(chain, use=None):
    """mean_cov_chain, src/utils.jl:96-111: (b, cov) as extended arrays; cov = 1/(Ngeneration*Npop) (flat .- b)(flat .- b)'."""
    Bk = backend(use)
    chain = np.asarray(chain, dtype=np.float64)
    Npop, Npar, Ngeneration = chain.shape
    c, pivot = _centred(Bk, chain)
    flat = c.transpose(1, 2, 0).reshape(Npar, Ngeneration * Npop)           # flatten_chain, :22-32
    b = _mean(flat, (1,))                                                   # :103
    dev = flat - b
    cov = np.dot(dev, dev.T) / (Ngeneration * Npop)                         # :104
    return (b + pivot.reshape(Npar, 1)).ravel(), cov


def mean_cov_chain(chain, use=None):
    b, cov = mean_cov_ext(chain, use)
    return to_float(b), to_float(cov)


def changed_per_chain(log_obj):
    """sum(diff(log_obj, dims = 2) .!= 0., dims = 2), utils.jl:61: an exact integer per chain.  The comparison is float64's own:
    a NaN difference (Inf - Inf) counts, 0.0 followed by -0.0 does not."""
    log_obj = np.asarray(log_obj, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (np.diff(log_obj, axis=1) != 0).sum(axis=1).astype(np.int64)


def accept_ratio(log_obj):
    """utils.jl:61: the count divided once by Ngeneration - 1 (two exact integers, one correctly rounded division)."""
    G = np.asarray(log_obj).shape[1]
    if G < 2:
        raise ValueError("the accept ratio needs at least 2 generations")
    return changed_per_chain(log_obj).astype(np.float64) / np.float64(G - 1)


# ---- tolerances ---------------------------------------------------------------------------------------------
RHAT_RTOL, MEAN_RTOL, COV_RTOL = 1e-9, 1e-12, 1e-9


def rhat_error(got, ref):
    """max over parameters of |got - ref| / ref: the tolerance is RHAT_RTOL."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / ref))


def mean_error(got, ref_mean, ref_cov):
    """max over p of |got_p - mean_p| / (|mean_p| + sd_p): the tolerance is MEAN_RTOL."""
    sd = np.sqrt(np.diag(ref_cov))
    scale = np.abs(ref_mean) + sd
    return float(np.max(np.abs(np.asarray(got) - ref_mean) / scale))


def cov_error(got, ref_cov):
    """max over (p, q) of |got_pq - C_pq| / sqrt(C_pp C_qq): the tolerance is COV_RTOL."""
    sd = np.sqrt(np.diag(ref_cov))
    return float(np.max(np.abs(np.asarray(got) - ref_cov) / np.outer(sd, sd)))
