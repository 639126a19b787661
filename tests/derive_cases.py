"""Derive programs (demcz_derive) shared by test_derive_program.py (no GPU) and test_gpu_derive.py, each with

  * its HIP C++ text,
  * a NumPy restatement: THE SAME OPERATIONS IN THE SAME ORDER on float64 arrays (chain N x d x G, log_obj N x G or None) giving
    the N x m x G column-major result, and
  * a per-draw function on Python floats (x, logp, data) -> list of m, the plain reading of the text that the restatements are
    checked against.

The programs compiled with -ffp-contract=off that use only +, -, *, comparisons and selects are IEEE operations one by one, so
their restatements are identical bit for bit (a NaN's sign and payload aside).  TRANSCENDENTAL uses exp, log1p, sqrt and /: it is
compared at REL_TOL, the tolerance tests/test_gpu_program_target.py::test_logistic_regression_logp_matches_numpy holds the device's
transcendentals to against the host's."""
import math

import numpy as np

REL_TOL = 1e-13


def _logp(chain, log_obj):
    N, _, G = chain.shape
    return np.full((N, G), np.nan) if log_obj is None else np.asarray(log_obj, dtype=np.float64)


# ---- GENERIC: any d, any m.  Column k: a weighted sum in a fixed order; k % 3 == 1: a select on x[0] > 0; k % 3 == 2: minus logp
GENERIC = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    for (int k = 0; k < DEMCZ_M; ++k) {
        double s = 0.5 * (double)(k + 1);
        for (int p = 0; p < DEMCZ_D; ++p) s = s + x[p] * (double)(p + k + 1);
        if (k % 3 == 1) s = (x[0] > 0.0) ? s : -s;
        if (k % 3 == 2) s = s - logp;
        out[k] = s;
    }
}
"""


def generic_numpy(m):
    def f(chain, log_obj, data=None):
        N, d, G = chain.shape
        lp = _logp(chain, log_obj)
        out = np.empty((N, m, G), order="F")
        with np.errstate(all="ignore"):
            for k in range(m):
                s = np.full((N, G), 0.5 * float(k + 1))
                for p in range(d):
                    s = s + chain[:, p, :] * float(p + k + 1)
                if k % 3 == 1:
                    s = np.where(chain[:, 0, :] > 0.0, s, -s)
                if k % 3 == 2:
                    s = s - lp
                out[:, k, :] = s
        return out
    return f


def generic_draw(m):
    def f(x, logp, data=None):
        out = []
        for k in range(m):
            s = 0.5 * float(k + 1)
            for p in range(len(x)):
                s = s + x[p] * float(p + k + 1)
            if k % 3 == 1:
                s = s if x[0] > 0.0 else -s
            if k % 3 == 2:
                s = s - logp
            out.append(s)
        return out
    return f


# ---- FIRST_ONLY: writes out[0] and nothing else (the other columns stay NaN)
FIRST_ONLY = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = x[0] + x[DEMCZ_D - 1];
}
"""


def first_only_numpy(m):
    def f(chain, log_obj, data=None):
        N, d, G = chain.shape
        out = np.full((N, m, G), np.nan, order="F")
        with np.errstate(all="ignore"):
            out[:, 0, :] = chain[:, 0, :] + chain[:, d - 1, :]
        return out
    return f


def first_only_draw(m):
    return lambda x, logp, data=None: [x[0] + x[-1]] + [math.nan] * (m - 1)


# ---- WITH_DATA / WITH_CONSTANTS: d >= 2, m = 3; the same arithmetic on data[0..3] and on the literals below
DATA_VALUES = (1.5, -0.25, 0.75, 3.0)
WITH_DATA = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = x[0] * data[0] + data[1];
    out[1] = (x[1] - data[2]) * data[3];
    out[2] = (double)ndata;
}
"""
WITH_CONSTANTS = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = x[0] * 1.5 + -0.25;
    out[1] = (x[1] - 0.75) * 3.0;
    out[2] = (data == nullptr) ? 4.0 : -1.0;
}
"""


def with_data_numpy(chain, log_obj, data=DATA_VALUES):
    N, d, G = chain.shape
    out = np.empty((N, 3, G), order="F")
    with np.errstate(all="ignore"):
        out[:, 0, :] = chain[:, 0, :] * data[0] + data[1]
        out[:, 1, :] = (chain[:, 1, :] - data[2]) * data[3]
    out[:, 2, :] = float(len(data))
    return out


def with_data_draw(x, logp, data=DATA_VALUES):
    return [x[0] * data[0] + data[1], (x[1] - data[2]) * data[3], float(len(data))]


# ---- SECOND: d = 3 (the three columns of a first derive), m = 2; a contrast, and whether logp is a number
SECOND = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = x[0] - x[2] * 2.0;
    out[1] = (logp == logp) ? 1.0 : 0.0;
}
"""


def second_numpy(chain, log_obj, data=None):
    N, d, G = chain.shape
    lp = _logp(chain, log_obj)
    out = np.empty((N, 2, G), order="F")
    with np.errstate(all="ignore"):
        out[:, 0, :] = chain[:, 0, :] - chain[:, 2, :] * 2.0
    out[:, 1, :] = np.where(lp == lp, 1.0, 0.0)
    return out


def second_draw(x, logp, data=None):
    return [x[0] - x[2] * 2.0, 1.0 if logp == logp else 0.0]


# ---- TRANSCENDENTAL: d >= 2, m = 3; a variance from a log-variance, a softplus, a ratio (exp, log1p, sqrt, /)
TRANSCENDENTAL = """
__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    out[0] = exp(x[0]);
    out[1] = log1p(exp(x[1]));
    out[2] = sqrt(x[0] * x[0] + 1.0) / (1.0 + exp(x[1]));
}
"""


def transcendental_numpy(chain, log_obj, data=None):
    N, d, G = chain.shape
    out = np.empty((N, 3, G), order="F")
    x0, x1 = chain[:, 0, :], chain[:, 1, :]
    out[:, 0, :] = np.exp(x0)
    out[:, 1, :] = np.log1p(np.exp(x1))
    out[:, 2, :] = np.sqrt(x0 * x0 + 1.0) / (1.0 + np.exp(x1))
    return out


def transcendental_draw(x, logp, data=None):
    return [math.exp(x[0]), math.log1p(math.exp(x[1])), math.sqrt(x[0] * x[0] + 1.0) / (1.0 + math.exp(x[1]))]


# (name, text, d, m, data, NumPy restatement, per-draw function, bit-exact?)
CASES = [
    ("generic_1_1", GENERIC, 1, 1, None, generic_numpy(1), generic_draw(1), True),
    ("generic_3_2", GENERIC, 3, 2, None, generic_numpy(2), generic_draw(2), True),
    ("generic_5_3", GENERIC, 5, 3, None, generic_numpy(3), generic_draw(3), True),
    ("generic_2_1", GENERIC, 2, 1, None, generic_numpy(1), generic_draw(1), True),
    ("generic_32_32", GENERIC, 32, 32, None, generic_numpy(32), generic_draw(32), True),
    ("first_only", FIRST_ONLY, 4, 3, None, first_only_numpy(3), first_only_draw(3), True),
    ("with_data", WITH_DATA, 3, 3, DATA_VALUES, with_data_numpy, with_data_draw, True),
    ("with_constants", WITH_CONSTANTS, 3, 3, None, with_data_numpy, with_data_draw, True),
    ("second", SECOND, 3, 2, None, second_numpy, second_draw, True),
    ("transcendental", TRANSCENDENTAL, 2, 3, None, transcendental_numpy, transcendental_draw, False),
]

SYNTAX_ERROR = """__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)
{
    double s = x[0];
    s = s + undefined_thing;
    out[0] = s;
}
"""

NO_ENTRY_POINT = "__device__ double f(const double* x) { return x[0]; }\n"


def program(demc, name):
    """The DerivedProgram of a case, and its restatement."""
    for n, text, d, m, data, f, _, _ in CASES:
        if n == name:
            return demc.DerivedProgram(text, d, m, data=data), f
    raise KeyError(name)


def generic_program(demc, d, m):
    return demc.DerivedProgram(GENERIC, d, m), generic_numpy(m)


def history(N, d, G, seed, with_log_obj=True):
    """A seeded N x d x G column-major history of standard normals and an N x G log_obj."""
    r = np.random.default_rng(seed)
    chain = np.asfortranarray(r.standard_normal((N, d, G)))
    log_obj = np.asfortranarray(-0.5 * r.standard_normal((N, G)) ** 2) if with_log_obj else None
    return chain, log_obj
