"""The worlds and schedules of the small-dimension tests (no GPU, no assertions).

At d = 2..5 a chain is a wave of one of three kernels: window_kernel_ps2 (regular launches of a handle with one chain to a wave),
window_kernel_ps2d (regular launches of a handle with two chains to a wave, DEMCZ_PS_DUAL) and the general window_kernel_ps
(everything else), each x d x LIVE x TEMPER with constants of its own (demcz_kernels_ps2.h: the row stride, the fields of a
pass's DMA, the temperature field).  Here: per d one world for each kind of handle, a schedule of demcz_run calls ("pieces") that
reaches every form on ONE handle, and the counts of the accept / reject outcomes of a pass per form -- and, with two chains to a
wave, per half of the wave -- what tests/test_small_wave_cases.py checks from the oracle alone and tests/test_gpu_small_wave.py
compares the library with.  Further: the worlds of the replicated consumer window_kernel_pc8 (d = 2..10, four forms) and a few
named edges.

Which kernel a piece runs (demcz_capi.hip: demcz_run, ps2_applicable, window_kernel_of; K = 10):
  * regular: K, the distance to the next boundary (K - (g_from - 1) % K) and the length are multiples of five, the length >= 5;
  * one chain to a wave: a piece is ONE launch when it follows a piece shorter than K (dimension_cases' docstring); regular ->
    window_kernel_ps2, otherwise window_kernel_ps; LIVE: a generation behind a K boundary inside the piece;
  * two chains to a wave: a regular launch runs window_kernel_ps2d as far as whole passes go; anything else runs window_kernel_ps
    one launch per K-window, never LIVE (dual_launches below);
  * tempered: the call has a temperature array (at most arena_gens = 1024 values here: it lies in the arena).
"""
import numpy as np

import demc_jl_amd as demc
import dimension_cases as dc

PASS, K = dc.PASS, dc.K
DIMS = (2, 3, 4, 5)
# jumps at which a little more than half of the proposals are accepted (the workload's 2.38 leaves most outcomes of a pass unseen)
GAMMA = {2: 0.9, 3: 0.7, 4: 0.55, 5: 0.45}
N_ONE, N_DUAL = 192, 193          # (odd: the last wave's second half shadows the last chain and writes nothing)

STEADY_LIVE_PLAIN, STEADY_LIVE_TEMPERED = "steady LIVE plain", "steady LIVE tempered"
STEADY_SHORT_PLAIN, STEADY_SHORT_TEMPERED = "steady non-LIVE plain", "steady non-LIVE tempered"
GENERAL_LIVE_PLAIN, GENERAL_LIVE_TEMPERED = "general LIVE plain", "general LIVE tempered"
GENERAL_SHORT_PLAIN, GENERAL_SHORT_TEMPERED = "general non-LIVE plain", "general non-LIVE tempered"
ONE_FORMS = (STEADY_LIVE_PLAIN, STEADY_LIVE_TEMPERED, STEADY_SHORT_PLAIN, STEADY_SHORT_TEMPERED,
             GENERAL_LIVE_PLAIN, GENERAL_LIVE_TEMPERED, GENERAL_SHORT_PLAIN, GENERAL_SHORT_TEMPERED)
# (a two-chain handle never runs the general kernel across a boundary)
DUAL_FORMS = (STEADY_LIVE_PLAIN, STEADY_LIVE_TEMPERED, STEADY_SHORT_PLAIN, STEADY_SHORT_TEMPERED,
              GENERAL_SHORT_PLAIN, GENERAL_SHORT_TEMPERED)
GENERAL_FORMS = (GENERAL_LIVE_PLAIN, GENERAL_LIVE_TEMPERED, GENERAL_SHORT_PLAIN, GENERAL_SHORT_TEMPERED)


def regular(g_from, g_to, k=K):
    n, to_boundary = g_to - g_from + 1, k - (g_from - 1) % k
    return k % PASS == 0 and to_boundary % PASS == 0 and n % PASS == 0 and n >= PASS


def form_of(g_from, g_to, tempered, k=K):
    """The form of a piece that is one launch (one chain to a wave)."""
    live = (g_to - 1) // k > (g_from - 1) // k
    return "%s %s %s" % ("steady" if regular(g_from, g_to, k) else "general", "LIVE" if live else "non-LIVE",
                         "tempered" if tempered else "plain")


def dual_launches(g_from, g_to, k=K):
    """The launches a two-chain handle makes of a piece whose regular launches are not cut for want of prepared draws (they
    follow a launch shorter than K): [(first generation, last generation, steady, live)]."""
    out, g = [], g_from
    while g <= g_to:
        boundary = ((g - 1) // k + 1) * k
        rest = g_to - g + 1
        if k % PASS == 0 and (boundary - g + 1) % PASS == 0 and rest >= PASS:
            e = g + rest // PASS * PASS - 1
            out.append((g, e, True, (e - 1) // k > (g - 1) // k))
        else:
            e = min(boundary, g_to)
            out.append((g, e, False, False))
        g = e + 1
    return out


def dual_form_of(g_from, g_to, tempered, k=K):
    """The form of a piece of a two-chain handle all of whose launches run the same kernel (what the schedule below consists of)."""
    steady, live = dual_launches(g_from, g_to, k)[-1][2:]
    return "%s %s %s" % ("steady" if steady else "general", "LIVE" if live else "non-LIVE", "tempered" if tempered else "plain")


def kernel_name(d, form, dual=False):
    steady, live, tempered = form.split()
    fn = ("window_kernel_ps2d" if dual else "window_kernel_ps2") if steady == "steady" else "window_kernel_ps"
    return "demcz::%s<MVNORMAL, %d, %s, %s>" % (fn, d, "true" if live == "LIVE" else "false", "true" if tempered == "tempered" else "false")


FIVES = [(5, False), (5, True)]
# two K-windows cut 2 + 5 + 3 and 1 + 5 + 4: the general kernel inside a window, a full pass in the middle, passes of 1..4
WINDOW_PAIR = (2, 5, 3, 1, 5, 4)
# two K-windows cut 3 + 5 + 6 + 2 + 4: the third piece crosses the boundary with fewer than five generations behind it
CROSSING_PAIR = (3, 5, 6, 2, 4)


def _pieces(lengths, form):
    pieces, g = [], 1
    for n, tempered in lengths:
        pieces.append((g, g + n - 1, tempered, form(g, g + n - 1, tempered)))
        g += n
    return pieces


def one_schedule():
    """[(g_from, g_to, tempered, form)], tiling 1..500, one chain to a wave.  The pieces of dimension_cases.pw_schedule (regular
    and general LIVE launches of 40 and 43 generations, plain and tempered, each behind a short piece); regular five-generation
    pieces; window pairs; and a second pair of regular LIVE launches late in the run, where the population no longer rejects as
    the starting one does."""
    lengths = [(b - a + 1, t) for a, b, t, _ in dc.pw_schedule()[:11]]             # ..200
    lengths += FIVES * 6                                                             # ..260
    for i in range(8):                                                               # ..420
        lengths += [(n, i % 2 == 1) for n in WINDOW_PAIR]
    lengths += [(5, False), (40, False), (5, True), (30, True)]                      # 426..465 and 471..500: regular LIVE
    return _pieces(lengths, form_of)


def dual_schedule():
    """The same for a handle with two chains to a wave: regular LIVE launches of 40 generations early and of 40 and 50 late, regular
    five-generation pieces, window pairs and crossing pairs (the general kernel, one launch per K-window)."""
    lengths = FIVES + [(40, False), (5, False), (40, True), (5, True)]              # ..100
    lengths += FIVES * 6                                                             # ..160
    for i in range(8):                                                               # ..320
        lengths += [(n, i % 2 == 1) for n in WINDOW_PAIR]
    for i in range(4):                                                               # ..400
        lengths += [(n, i % 2 == 1) for n in CROSSING_PAIR]
    lengths += [(5, False), (40, False), (5, True), (50, True)]                      # 406..445 and 451..500: regular LIVE
    return _pieces(lengths, dual_form_of)


def small_case(d, dual):
    """The world of d in 2..5 for a handle with one (dual = False) or two chains to a wave."""
    N = N_DUAL if dual else N_ONE
    pieces = dual_schedule() if dual else one_schedule()
    G = pieces[-1][1]
    return dict(kind="mvn", d=d, dual=dual, N=N, K=K, seed=20261019 + 1000 * d + dual, gamma=GAMMA[d],
                problem=demc.workloads.mvnormal_problem(d, N), pieces=pieces, G=G, temperature=dc.temperatures(G))


def launches_after(case):
    """The count of window launches behind every piece."""
    out, n = [], 0
    for a, b, _, _ in case["pieces"]:
        n += len(dual_launches(a, b, case["K"])) if case["dual"] else 1
        out.append(n)
    return out


def halves(case):
    """The chain subsets whose outcomes are held separately: with two chains to a wave the even-indexed chains (lanes 0..31) and
    the odd-indexed ones (lanes 32..63)."""
    if not case["dual"]:
        return {"all": None}
    return {"even": np.arange(0, case["N"], 2), "odd": np.arange(1, case["N"], 2)}


# ---- the replicated consumer, window_kernel_pc8 ------------------------------------------------------------------------------------
PC8_TARGETS = tuple(("mvn", d) for d in range(2, 11)) + (("iso", 10),)
PC8_GAMMA = {("mvn", 2): 0.9, ("mvn", 3): 0.7, ("mvn", 4): 0.55, ("mvn", 5): 0.45, ("mvn", 6): 0.4, ("mvn", 7): 0.35, ("mvn", 8): 0.3,
             ("mvn", 9): 0.3, ("mvn", 10): 0.25, ("iso", 10): 1.2}
PC8_FORMS = ("LIVE plain", "LIVE tempered", "non-LIVE plain", "non-LIVE tempered")


def pc8_schedule():
    """[(g_from, g_to, tempered, form)], tiling 1..60: a piece inside a window, then a long one across boundaries, plain and
    tempered (pc8 resolves one generation at a time: no regularity, no passes)."""
    def form(a, b, tempered):
        return "%s %s" % ("LIVE" if (b - 1) // K > (a - 1) // K else "non-LIVE", "tempered" if tempered else "plain")
    return _pieces([(4, False), (23, False), (3, True), (27, True), (3, False)], form)


def pc8_kernel_name(kind, d, form):
    live, tempered = form.split()
    return "demcz::window_kernel_pc8<%s, %d, %s, %s>" % (dc.TARGET_NAME[kind], d, "true" if live == "LIVE" else "false",
                                                         "true" if tempered == "tempered" else "false")


def pc8_case(kind, d):
    N = 100
    w = (demc.workloads.mvnormal_problem if kind == "mvn" else demc.workloads.iso_quad_problem)(d, N)
    pieces = pc8_schedule()
    G = pieces[-1][1]
    return dict(kind=kind, d=d, N=N, K=K, seed=20261019 + 7 * d + (kind == "iso"), gamma=PC8_GAMMA[kind, d], problem=w,
                pieces=pieces, G=G, temperature=dc.temperatures(G))


def kernel_names_planned():
    """Every kernel name the tests of these worlds assert."""
    names = set()
    for d in DIMS:
        names |= {kernel_name(d, p[3], False) for p in one_schedule()} | {kernel_name(d, p[3], True) for p in dual_schedule()}
    for kind, d in PC8_TARGETS:
        names |= {pc8_kernel_name(kind, d, p[3]) for p in pc8_schedule()}
    return names


# ---- named edges: each one small world --------------------------------------------------------------------------------------------
def temps_with_zeros(G):
    """Zeros ((lp' - lp) / 0 = +-Inf accepts every improvement and nothing else, 0 / 0 = NaN rejects), with 2.5, 1e-300 and 1e300
    mixed in (the schedule of test_gpu_parity._temps_with_zeros)."""
    T = np.zeros(G)
    T[::7] = 2.5
    T[3::11] = 1e-300
    T[5::13] = 1e300
    return T


def edge_case(d, N, dual, lengths, k=K, temperature=None):
    form = (lambda a, b, t: dual_form_of(a, b, t, k)) if dual else (lambda a, b, t: form_of(a, b, t, k))
    pieces = _pieces(lengths, form)
    G = pieces[-1][1]
    return dict(kind="mvn", d=d, dual=dual, N=N, K=k, seed=20261019 + 31 * d + 7 * N + dual, gamma=GAMMA[d],
                problem=demc.workloads.mvnormal_problem(d, N), pieces=pieces, G=G,
                temperature=dc.temperatures(G) if temperature is None else temperature)


# A tempered call of 45 generations behind a call of 15, K = 5: the launch before prepared 15 generations of draws, so the call is
# cut there (demcz_run: (15 // K) * K) and its second launch starts 15 temperatures -- an odd number: 8 but not 16 bytes -- into
# the call's array.
CUT_LENGTHS, CUT_K, CUT_LAUNCHES = [(15, False), (45, True)], 5, [1, 3]
TINY_LENGTHS = [(5, False), (20, True), (5, True), (20, False)]       # every steady form
TINY_POPULATIONS = {False: (1, 5), True: (1, 9)}                       # idle chain waves in a workgroup; a wave whose second half shadows
