"""Program texts and small builders shared by the program-target tests of the wave-per-chain layout
(test_program_wave.py, test_gpu_program_wave.py): restatements of the built-in targets (ISO, MVN, LINREG), a target with no
built-in (ROSENBROCK) and one that calls the device library's transcendentals (LOGISTIC); and four programs that leave the finite
numbers or the straight line (BOX, SQRTDOM, POLE, TRIPS: test_gpu_nonfinite.py), each written with + - * /, comparisons and sqrt
only -- compiled with contraction off, its Python twin in plain floats performs the same IEEE operations in the same order."""
import math

import numpy as np

import demc_jl_amd as demc

ISO = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) {
        const double r = x[i] - data[i];
        q = (i == 0) ? r * r : fma(r, r, q);
    }
    return -q;
}
"""

# data = mu (d) || W packed row-major lower triangle (row i at i(i+1)/2) || c0: the order of target_logp's full-block MvNormal
MVN = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const double* W = data + DEMCZ_D;
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) {
        const double* wrow = W + (i * (i + 1)) / 2;
        double acc = wrow[0] * (x[0] - data[0]);
        for (int j = 1; j <= i; ++j) acc = fma(wrow[j], x[j] - data[j], acc);
        q = (i == 0) ? acc * acc : fma(acc, acc, q);
    }
    return fma(-0.5, q, data[DEMCZ_D + (DEMCZ_D * (DEMCZ_D + 1)) / 2]);
}
"""

# data = design (nobs x d, row-major) || y: the regression SSE in the spec's sixteen interleaved partial sums and fixed tree
LINREG = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int64_t nobs = ndata / (DEMCZ_D + 1);
    const double* y = data + nobs * DEMCZ_D;
    double part[16];
    for (int l = 0; l < 16; ++l) part[l] = 0.0;
    const int64_t nfull = nobs / 16;
    for (int64_t k = 0; k < nfull; ++k) {
        for (int l = 0; l < 16; ++l) {
            const double* row = data + (k * 16 + l) * DEMCZ_D;
            double acc = row[0] * x[0];
            for (int j = 1; j < DEMCZ_D; ++j) acc = fma(row[j], x[j], acc);
            const double r = y[k * 16 + l] - acc;
            part[l] = (k == 0) ? r * r : fma(r, r, part[l]);
        }
    }
    for (int l = 0; l < 16; ++l) {
        const int64_t o = nfull * 16 + l;
        if (o < nobs) {
            const double* row = data + o * DEMCZ_D;
            double acc = row[0] * x[0];
            for (int j = 1; j < DEMCZ_D; ++j) acc = fma(row[j], x[j], acc);
            const double r = y[o] - acc;
            part[l] = (nfull == 0) ? r * r : fma(r, r, part[l]);
        }
    }
    for (int h = 8; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) part[l] = part[l] + part[l + h];
    return -0.5 * part[0];
}
"""

ROSENBROCK = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double s = 0.0;
    for (int i = 0; i + 1 < DEMCZ_D; ++i) {
        const double a = x[i + 1] - x[i] * x[i];
        const double b = 1.0 - x[i];
        s = s + 100.0 * (a * a) + b * b;
    }
    return -s;
}
"""

# data = design (nobs x d, row-major) || labels
LOGISTIC = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int64_t nobs = ndata / (DEMCZ_D + 1);
    const double* y = data + nobs * DEMCZ_D;
    double s = 0.0;
    for (int64_t o = 0; o < nobs; ++o) {
        double eta = 0.0;
        for (int j = 0; j < DEMCZ_D; ++j) eta = eta + data[o * DEMCZ_D + j] * x[j];
        s = s + (y[o] * eta - log1p(exp(eta)));
    }
    return s;
}
"""

SYNTAX_ERROR = """__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double s = x[0];
    s = s + undefined_thing;
    return -s;
}
"""


def iso_program(mu):
    return demc.ProgramTarget(ISO, len(mu), data=mu)


def mvn_program(mu, W, c0):
    d = len(mu)
    wp = np.concatenate([np.asarray(W)[i, :i + 1] for i in range(d)])
    return demc.ProgramTarget(MVN, d, data=np.concatenate([mu, wp, [c0]]))


def linreg_program(design, y):
    design = np.asarray(design, dtype=np.float64)
    return demc.ProgramTarget(LINREG, design.shape[1], data=np.concatenate([np.ascontiguousarray(design).ravel(), y]))


def logistic_program(design, labels):
    design = np.asarray(design, dtype=np.float64)
    return demc.ProgramTarget(LOGISTIC, design.shape[1], data=np.concatenate([np.ascontiguousarray(design).ravel(), labels]))


def rosenbrock_closure(x):
    s = 0.0
    for i in range(len(x) - 1):
        a = x[i + 1] - x[i] * x[i]
        b = 1.0 - x[i]
        s = s + 100.0 * (a * a) + b * b
    return -s


# ---- programs that return non-finite values or branch on their argument, and their Python twins --------------------------------
# data = c (d) || h (d): the isotropic quadratic inside the box |x_i - c_i| <= h_i, -inf outside -- the return leaves the loop at
# the first violation, so on the wave layout the lanes of a wavefront (one candidate each) leave it at different trips.
# (Written as two comparisons: a NaN residual is no violation and comes out as a NaN sum, so an infinite box is the plain quadratic.)
BOX = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) {
        const double r = x[i] - data[i];
        const double h = data[DEMCZ_D + i];
        if (r > h || -r > h) return -INFINITY;
        q = (i == 0) ? r * r : r * r + q;
    }
    return -q;
}
"""

# data = a, b: -(sqrt(x[0] - a) - b)^2 - sum_{i >= 1} x_i^2: NaN, by arithmetic, where x[0] < a
SQRTDOM = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const double t = sqrt(x[0] - data[0]) - data[1];
    double s = t * t;
    for (int i = 1; i < DEMCZ_D; ++i) s = s + x[i] * x[i];
    return -s;
}
"""

# data = t: +inf where x[1] > t, the isotropic quadratic about 0 elsewhere.  A chain that accepts +inf stays: every later
# difference is -inf or NaN.
POLE = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    if (x[1] > data[0]) return INFINITY;
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) q = q + x[i] * x[i];
    return -q;
}
"""

# a loop whose length (0..7) depends on x[0]; for finite x only ((int) of a non-finite value is undefined)
TRIPS = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int n = ((int)(fabs(x[0]) * 8.0)) & 7;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s = s * 0.5 + x[k % DEMCZ_D] * x[k % DEMCZ_D];
    double q = 0.0;
    for (int i = 0; i < DEMCZ_D; ++i) q = q + x[i] * x[i];
    return -s - q;
}
"""


def box_program(c, h):
    return demc.ProgramTarget(BOX, len(c), data=np.concatenate([c, h]))


def box_closure(c, h):
    c, h = [float(v) for v in c], [float(v) for v in h]

    def logobj(x):
        q = 0.0
        for i in range(len(c)):
            r = x[i] - c[i]
            if r > h[i] or -r > h[i]:
                return -math.inf
            q = r * r if i == 0 else r * r + q
        return -q
    return logobj


def sqrtdom_program(d, a, b):
    return demc.ProgramTarget(SQRTDOM, d, data=[a, b])


def sqrtdom_closure(d, a, b):
    a, b = float(a), float(b)

    def logobj(x):
        v = x[0] - a
        t = (math.sqrt(v) if v >= 0.0 else math.nan) - b          # (math.sqrt raises where IEEE's returns NaN; NaN >= 0 is false)
        s = t * t
        for i in range(1, d):
            s = s + x[i] * x[i]
        return -s
    return logobj


def pole_program(d, t):
    return demc.ProgramTarget(POLE, d, data=[t])


def pole_closure(d, t):
    t = float(t)

    def logobj(x):
        if x[1] > t:
            return math.inf
        q = 0.0
        for i in range(d):
            q = q + x[i] * x[i]
        return -q
    return logobj


def trips_program(d):
    return demc.ProgramTarget(TRIPS, d)


def trips_closure(d):
    def logobj(x):
        n = int(abs(x[0]) * 8.0) & 7
        s = 0.0
        for k in range(n):
            s = s * 0.5 + x[k % d] * x[k % d]
        q = 0.0
        for i in range(d):
            q = q + x[i] * x[i]
        return -s - q
    return logobj
