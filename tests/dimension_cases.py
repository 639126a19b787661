"""The worlds and schedules of the every-dimension tests (no GPU, no assertions).

window_kernel_pw is built for every d = 6..32 in six forms per target, the sixteen-lane regression kernel for every d = 2..28
with and without helper waves; each dimension compiles generated text and constants of its own.  Here: for every such (target, d)
one small world and a schedule of demcz_run calls ("pieces") that reaches every form on ONE handle, the oracle's run of it, and
the count of the 32 accept / reject outcomes of a five-generation pass per form -- what tests/test_dimension_cases.py checks from
the oracle alone and tests/test_gpu_every_dimension.py compares the library with.

Which form a piece runs (demcz_capi.hip: demcz_run, pw_regular, window_kernel_of; K = 10, a handle that can go LIVE):
  * a piece is ONE launch when the draws of its length are not already there: the launch before prepares as many generations of
    draws as ITS call was long, and a longer call behind a call of K generations or more would be cut at that many -- so every
    long piece here follows a piece shorter than K;
  * LIVE: a K boundary lies inside the launch with a generation behind it -- (g_to - 1) // K > (g_from - 1) // K;
  * REG: LIVE, and K, K - (g_from - 1) % K and the length are multiples of five;
  * tempered: the call has a temperature array.
"""
import numpy as np

import demc_jl_amd as demc

PASS = 5                      # generations per pass of the wave-per-chain kernels (PS_R, demcz_kernels_ps.h)
K = 10
PW_DIMS = tuple(range(6, 33))
LR_DIMS = tuple(range(2, 29))
ML_COOP_MAX_OBS = 1536        # demcz_kernels_ml.h
TAIL_PAIRS = 7                # five-generation pieces behind the long ones: with those between them ten per non-LIVE form

REG_PLAIN, REG_TEMPERED = "REG LIVE plain", "REG LIVE tempered"
LIVE_PLAIN, LIVE_TEMPERED = "general LIVE plain", "general LIVE tempered"
SHORT_PLAIN, SHORT_TEMPERED = "non-LIVE plain", "non-LIVE tempered"
FORMS = (REG_PLAIN, REG_TEMPERED, LIVE_PLAIN, LIVE_TEMPERED, SHORT_PLAIN, SHORT_TEMPERED)
# the template arguments behind <TARGET, d, ...> in demcz_debug_kernel_name (tests/golden/kernel_choice.json, wave_mvn_d6)
FORM_SUFFIX = {REG_PLAIN: "true, false, false, true", REG_TEMPERED: "true, true, false, true", LIVE_PLAIN: "true, false",
               LIVE_TEMPERED: "true, true", SHORT_PLAIN: "false, false", SHORT_TEMPERED: "false, true"}
TARGET_NAME = {"mvn": "MVNORMAL", "iso": "ISO_QUAD"}
# jumps at which about half of the proposals are accepted in these worlds (the workloads' 2.38 leaves most outcomes unseen)
PW_GAMMA = {"mvn": 0.2, "iso": 1.2}


def form_of(g_from, g_to, tempered, k=K):
    """The form the rules in this module's docstring give a piece that is one launch."""
    live = (g_to - 1) // k > (g_from - 1) // k
    n, to_boundary = g_to - g_from + 1, k - (g_from - 1) % k
    reg = live and k % PASS == 0 and to_boundary % PASS == 0 and n % PASS == 0
    if reg:
        return REG_TEMPERED if tempered else REG_PLAIN
    if live:
        return LIVE_TEMPERED if tempered else LIVE_PLAIN
    return SHORT_TEMPERED if tempered else SHORT_PLAIN


def pw_kernel_name(kind, d, form):
    return "demcz::window_kernel_pw<%s, %d, %s>" % (TARGET_NAME[kind], d, FORM_SUFFIX[form])


def pw_schedule():
    """[(g_from, g_to, tempered, form)], tiling 1..G.  Four long pieces, each behind a short one: 40 generations from a multiple
    of five (REG), plain and tempered; 43 generations (no multiple of five) from a window's start and 43 from the middle of a
    window (general LIVE), plain and tempered.  Around and behind them five-generation pieces inside one window, alternately plain
    and tempered: a full pass each."""
    lengths = [(5, False), (5, True),
               (40, False),                 # 11..50: REG
               (5, False),
               (40, True),                  # 56..95: REG, from the middle of a window
               (5, True),
               (43, False),                 # 101..143: general (the length)
               (5, False),
               (43, True),                  # 149..191: general (starts and ends inside a window)
               (5, True), (4, False)]       # ..200
    lengths += [(5, False), (5, True)] * TAIL_PAIRS
    pieces, g = [], 1
    for n, tempered in lengths:
        pieces.append((g, g + n - 1, tempered, form_of(g, g + n - 1, tempered)))
        g += n
    return pieces


def temperatures(G, hot=3.0, cold=0.5):
    """A mild geometric schedule: acceptance stays up at both ends."""
    return hot * (cold / hot) ** (np.arange(G) / max(G - 1, 1))


def pw_case(kind, d):
    """The world of (kind in {"mvn", "iso"}, d in 6..32): problem, N, K, seed, gamma, the schedule and its temperatures."""
    N = 96
    w = (demc.workloads.mvnormal_problem if kind == "mvn" else demc.workloads.iso_quad_problem)(d, N)
    pieces = pw_schedule()
    G = pieces[-1][1]
    return dict(kind=kind, d=d, N=N, K=K, seed=20261019 + 100 * d + (kind == "iso"), gamma=PW_GAMMA[kind], problem=w,
                pieces=pieces, G=G, temperature=temperatures(G))


def passes_of(g_from, g_to, k=K):
    """The passes the wave-per-chain kernels form of a piece: five generations, cut at K boundaries and
    at the piece's end.  [(first generation, last generation)]."""
    out, g = [], g_from
    while g <= g_to:
        e = min(g + PASS - 1, ((g - 1) // k + 1) * k, g_to)
        out.append((g, e))
        g = e + 1
    return out


def pass_outcomes(pieces, log_obj, lp0, k=K, forms=FORMS, length=PASS, chains=None):
    """{form: counts[2 ** length]} over the passes of `length` generations (the full ones: five) of every form's pieces, of all
    chains or of the subset `chains`.  A pass's outcome: the bits log_obj[g] != log_obj[g - 1], the first generation's the highest
    (generation 0 is the starting log-density lp0)."""
    lo = np.concatenate([np.asarray(lp0, dtype=np.float64)[:, None], np.asarray(log_obj)], axis=1)      # column g = generation g
    if chains is not None:
        lo = lo[chains]
    moved = lo[:, 1:] != lo[:, :-1]                                                                     # column g - 1 = generation g
    counts = {f: np.zeros(1 << length, dtype=np.int64) for f in forms}
    for g_from, g_to, _, form in pieces:
        for a, b in passes_of(g_from, g_to, k):
            if b - a + 1 == length:
                code = (moved[:, a - 1:b] * (1 << np.arange(length - 1, -1, -1))).sum(axis=1)
                counts[form] += np.bincount(code, minlength=1 << length)
    return counts


def ml_coop_resident_tiles(d):
    """demcz_kernels_ml.h, ml_coop_resident_tiles: whole 64-observation rounds of the design that stay in the 100 KB of LDS
    (ML_COOP_RES_BYTES / (64 rows * d * 8 bytes)), at most all ML_COOP_MAX_OBS / 64 of them."""
    return min(102400 // (512 * d), ML_COOP_MAX_OBS // 64)


def lr_case(d, coop):
    """The regression world of d in 2..28.  COOP (helper waves, at most ML_COOP_MAX_OBS observations): resident full rounds, a
    further full round (not resident wherever fewer than 23 are), a last round of 37 observations.  Otherwise 1601 observations.
    22 chains: the last chain wave of four is half filled.  Two pieces cut inside a window, plain then tempered."""
    nobs = 64 * min(ml_coop_resident_tiles(d), 22) + 101 if coop else 1601
    N, G = 22, 25
    w = demc.workloads.linreg_problem(d, N, nobs=nobs)
    pieces = [(1, 13, False), (14, G, True)]
    return dict(d=d, coop=coop, nobs=nobs, N=N, K=K, seed=20261019 + d, gamma=w["gamma"], problem=w, pieces=pieces, G=G,
                temperature=temperatures(G))


def lr_kernel_name(d, coop, lr16_fits=True):
    """What the library launches for the regression target on sixteen lanes per chain.  d = 10 has a kernel of its own while design
    and observations fit LDS (window_kernel_lr16, the matrix instruction; up to 1472 observations): the COOP case's 1381
    observations run that one, and window_kernel_ml's helper-wave form is not chosen at d = 10 by any case here; 1601 observations
    do not fit and run window_kernel_ml<LINREG_SSE, 10, 16> like any other dimension.  lr16_fits = False: a count that does not
    fit window_kernel_lr16 -- from 1473 to ML_COOP_MAX_OBS observations that is the helper-wave form at d = 10 too
    (tests/full_update_cases.py)."""
    if d == 10 and coop and lr16_fits:
        return "demcz::window_kernel_lr16<10, false, false>"
    return "demcz::window_kernel_ml<LINREG_SSE, %d, 16%s>" % (d, ", false, false, true" if coop else "")


def oracle_run(O, case):
    """The oracle over the case's pieces.  dict(chain, log_obj, X, logp, Z, M, changed, lp0)."""
    w, N, d, G = case["problem"], case["N"], case["d"], case["G"]
    Z0 = w["Zinit"]
    M0 = Z0.shape[0]
    Mcap = M0 + N * (G // case["K"] + 1)
    prob = O.Problem(N, d, case["K"], Mcap, w["eps_scale"], case["seed"], target=w["target"].spec())
    X = np.array(Z0[M0 - N:], order="F")
    lp = O.logp(prob, X)
    lp0 = lp.copy()
    Z = np.zeros((Mcap, d), order="F")
    Z[:M0] = Z0
    chain, lobj, changed, M = np.zeros((N, d, G), order="F"), np.zeros((N, G), order="F"), np.zeros(G, dtype=np.int64), M0
    for p in case["pieces"]:
        a, b, tempered = p[0], p[1], p[2]
        M, ch, lo, cg = O.run(prob, X, lp, Z, M, a, b, case["gamma"], temperature=case["temperature"][a - 1:b] if tempered else None)
        chain[:, :, a - 1:b], lobj[:, a - 1:b], changed[a - 1:b] = ch, lo, cg
    return dict(chain=chain, log_obj=lobj, X=X, logp=lp, Z=Z[:M].copy(), M=M, changed=changed, lp0=lp0)
