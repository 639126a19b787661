"""Predictive programs (demcz_predict, demcz_ppc) shared by test_predict_program.py, test_predict_reference.py (no GPU) and
test_gpu_predict.py, each with its HIP C++ text and a NumPy restatement over tests/predict_reference.py's streams:

    f(chain N x d x w, log_obj N x w or None, streams of the N x w draws) -> N x m x w, column-major

The programs use +, -, *, comparisons, selects and exact integer-to-double conversions only (compiled with -ffp-contract=off), and
their random numbers are the stream's own: the restatements are the device's values bit for bit (a NaN's sign and payload aside)."""
import numpy as np

import predict_reference as pr

HEAD = "__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out)\n"


def _logp(chain, log_obj):
    N, _, w = chain.shape
    return np.full((N, w), np.nan) if log_obj is None else np.asarray(log_obj, dtype=np.float64)


# ---- (a) GENERIC: any d, any m.  Every seventh column starts a round of uniform, normal, uniform, normal, normal, bits, exponential:
# round 1 from the empty state   block 0 (word held), block 1 (normal held), the spare word, the spare normal, block 2 (normal
#                                held), block 3 (no spare touched), block 4 (word held);
# round 2 with both spares held  the spare word, the spare normal, block 5 (word held), block 6 (normal held), the spare normal,
#                                block 7, the spare word -- both empty again, and round 3 is round 1 from block 8.
GENERIC = HEAD + """{
    double v[7];
#pragma unroll
    for (int k = 0; k < DEMCZ_M; ++k) {
        if (k % 7 == 0) {
            uint64_t r1, r2;
            v[0] = demcz_uniform(rng);
            v[1] = demcz_normal(rng);
            v[2] = demcz_uniform(rng);
            v[3] = demcz_normal(rng);
            v[4] = demcz_normal(rng);
            demcz_bits(rng, &r1, &r2);
            v[5] = (double)(r1 >> 11) * 0x1p-53 - (double)(r2 >> 11) * 0x1p-53;
            v[6] = demcz_exponential(rng);
        }
        double s = x[k % DEMCZ_D] * v[k % 7] + v[(k + 3) % 7];
        if (k % 4 == 3) s = s - logp;
        out[k] = s;
    }
}
"""


def generic_numpy(m):
    def f(chain, log_obj, streams):
        N, d, w = chain.shape
        lp = _logp(chain, log_obj)
        out = np.empty((N, m, w), order="F")
        v = [None] * 7
        with np.errstate(all="ignore"):
            for k in range(m):
                if k % 7 == 0:
                    v[0] = streams.uniform()
                    v[1] = streams.normal()
                    v[2] = streams.uniform()
                    v[3] = streams.normal()
                    v[4] = streams.normal()
                    r1, r2 = streams.bits()
                    v[5] = pr.word_to_unit(r1) - pr.word_to_unit(r2)
                    v[6] = streams.exponential()
                s = chain[:, k % d, :] * v[k % 7] + v[(k + 3) % 7]
                if k % 4 == 3:
                    s = s - lp
                out[:, k, :] = s
        return out
    return f


# ---- ONE_UNIFORM: d = 2, m = 1; one uniform per draw (the stride-twice shape: the restatement stays cheap)
ONE_UNIFORM = HEAD + """{
    out[0] = x[0] + x[1] * demcz_uniform(rng);
}
"""


def one_uniform_numpy(chain, log_obj, streams):
    N, d, w = chain.shape
    out = np.empty((N, 1, w), order="F")
    out[:, 0, :] = chain[:, 0, :] + chain[:, 1, :] * streams.uniform()
    return out


# ---- (b) DIVERGENT: d = 1, m = 2; a loop whose trip count differs from lane to lane
DIVERGENT_CAP = 64
DIVERGENT = HEAD + """{
    int n = 0;
    double u;
    do { u = demcz_uniform(rng); ++n; } while (u < 0.75 && n < 64);
    out[0] = n;
    out[1] = u;
}
"""


def divergent_numpy(chain, log_obj, streams):
    N, d, w = chain.shape
    n = np.zeros((N, w), dtype=np.int64)
    u = np.zeros((N, w))
    active = np.ones((N, w), dtype=bool)
    while active.any():
        u = np.where(active, streams.uniform(active), u)
        n = n + active
        active = active & (u < 0.75) & (n < DIVERGENT_CAP)
    out = np.empty((N, 2, w), order="F")
    out[:, 0, :] = n.astype(np.float64)
    out[:, 1, :] = u
    return out


# ---- (c) COUNT8: d = 1, m = 2; how many of 8 uniforms are below 0.5 (integer-valued: ties with an observed count), and their sum
COUNT8 = HEAD + """{
    double n = 0.0, s = 0.0;
    for (int j = 0; j < 8; ++j) {
        const double u = demcz_uniform(rng);
        n = n + ((u < 0.5) ? 1.0 : 0.0);
        s = s + u;
    }
    out[0] = n;
    out[1] = s;
}
"""


def count8_numpy(chain, log_obj, streams):
    N, d, w = chain.shape
    n, s = np.zeros((N, w)), np.zeros((N, w))
    for _ in range(8):
        u = streams.uniform()
        n = n + np.where(u < 0.5, 1.0, 0.0)
        s = s + u
    out = np.empty((N, 2, w), order="F")
    out[:, 0, :], out[:, 1, :] = n, s
    return out


# ---- (d) SPECIALS: d = 1, m = 4; +-INFINITY, an output left unwritten, a NaN made on purpose, and a finite column
SPECIALS = HEAD + """{
    const double u = demcz_uniform(rng);
    out[0] = (u < 0.5) ? INFINITY : ((u < 0.75) ? -INFINITY : u);
    out[2] = (u < 0.25) ? NAN : ((u < 0.5) ? 0.0 : -0.0);
    out[3] = x[0] + demcz_normal(rng);
}
"""


def specials_numpy(chain, log_obj, streams):
    N, d, w = chain.shape
    u = streams.uniform()
    out = np.full((N, 4, w), np.nan, order="F")
    out[:, 0, :] = np.where(u < 0.5, np.inf, np.where(u < 0.75, -np.inf, u))
    out[:, 2, :] = np.where(u < 0.25, np.nan, np.where(u < 0.5, 0.0, -0.0))
    out[:, 3, :] = chain[:, 0, :] + streams.normal()
    return out


# (name, text, d, m, restatement)
CASES = [
    ("generic_1_1", GENERIC, 1, 1, generic_numpy(1)),
    ("generic_3_2", GENERIC, 3, 2, generic_numpy(2)),
    ("generic_32_32", GENERIC, 32, 32, generic_numpy(32)),
    ("generic_5_3", GENERIC, 5, 3, generic_numpy(3)),
    ("one_uniform", ONE_UNIFORM, 2, 1, one_uniform_numpy),
    ("divergent", DIVERGENT, 1, 2, divergent_numpy),
    ("count8", COUNT8, 1, 2, count8_numpy),
    ("specials", SPECIALS, 1, 4, specials_numpy),
]

SYNTAX_ERROR = HEAD + """{
    double s = demcz_normal(rng);
    s = s + undefined_thing;
    out[0] = s;
}
"""

NO_ENTRY_POINT = "__device__ double f(const double* x) { return x[0]; }\n"


def program(demc, name):
    """The PredictiveProgram of a case, and its restatement."""
    for n, text, d, m, f in CASES:
        if n == name:
            return demc.PredictiveProgram(text, d, m), f
    raise KeyError(name)


def generic_program(demc, d, m):
    return demc.PredictiveProgram(GENERIC, d, m), generic_numpy(m)


def reference(f, chain, log_obj, seed, g_from=1, chain_id0=0):
    """f over the window g_from .. g_from + w - 1 of chains chain_id0 .. chain_id0 + N - 1 with the streams the specification
    gives those draws."""
    N, _, w = chain.shape
    return f(chain, log_obj, pr.window_streams(seed, N, g_from, g_from + w - 1, chain_id0))
