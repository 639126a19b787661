"""Program texts and small builders shared by the program-target tests of the wave-per-chain layout
(test_program_wave.py, test_gpu_program_wave.py): restatements of the built-in targets (ISO, MVN, LINREG), a target with no
built-in (ROSENBROCK) and one that calls the device library's transcendentals (LOGISTIC)."""
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
