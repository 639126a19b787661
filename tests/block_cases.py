"""The worlds and schedules of the block-update tests (no GPU, no assertions).

Block updates (more than one block, or one block that is not 0..d-1 in order) run on kernels of their own (demcz_capi.hip:
mlb_kernel / mlb_fn, window_kernel_of):
  * window_kernel_mlb<MVNORMAL, D, L, REC, LIVE, QB, GM>, 8 lanes per chain at d = 5, 6, 10 and 16 at d = 20: fused (REC = false),
    split non-LIVE and split LIVE, each with the sums of the quadratic form ungrouped and cut by the group-start mask (GM: the blocks,
    in order, are consecutive index ranges covering 0..d-1) -- 24; the incremental form QB = 5 of d = 20 in four blocks of five,
    fused, split, split LIVE -- 3; four split forms on 32 lanes behind DEMCZ_MLB_L32 -- 31 instantiations;
  * window_kernel<TARGET, D, false>, one lane per chain: MvNormal 2, 3, 4, 5, 8, 10, 20 (a grouped and an ungrouped run-time path
    each), iso-quad 10, regression 10 and 26; window_kernel_generic<TARGET> at any other dimension; a program target's window_blocks.
Here: one world per kernel and block structure with a schedule of demcz_run calls ("pieces") that reaches every form on ONE handle,
the oracle's run of it, and the counts of the 2^NB accept / reject outcomes of a generation's block-steps per form -- what
tests/test_block_cases.py checks from the oracle alone and tests/test_gpu_block_forms.py compares the library with.

Which form a piece runs (demcz_run_plan.h; K = 5): a piece is one launch of the split layout when it follows a piece shorter than
K; it is LIVE when a K boundary lies inside it with a generation behind it; tempered when the call has a temperature array.  The
fused and the one-lane layouts launch once per K-window and have the plain and the tempered form only; their worlds run the same
schedule (calls cut inside a window and across boundaries).

demcz_debug_kernel_name reports the GM instantiations without their trailing arguments, so a reported name stands for two
instantiations; which of them ran follows from the world's block structure (grouped() below restates demcz_create's rule).
"""
import numpy as np

import demc_jl_amd as demc
from helpers import oracle_sample_logobj
from program_texts import ROSENBROCK, rosenbrock_closure

K = 5
N_MAIN = 96
MLB_MAX_BLOCKS = 64                       # demcz_kernels_ml.h
MI355X_CUS = 256                          # the CPU tier's stand-in for the device's CU count (the GPU tier reads the device)

LIVE_PLAIN, LIVE_TEMPERED, SHORT_PLAIN, SHORT_TEMPERED = "LIVE plain", "LIVE tempered", "non-LIVE plain", "non-LIVE tempered"
FORMS = (LIVE_PLAIN, LIVE_TEMPERED, SHORT_PLAIN, SHORT_TEMPERED)


def _r(a, b):
    return list(range(a, b))


def form_of(g_from, g_to, tempered, k=K):
    live = (g_to - 1) // k > (g_from - 1) // k
    return "%s %s" % ("LIVE" if live else "non-LIVE", "tempered" if tempered else "plain")


def pieces_of(lengths, k=K):
    pieces, g = [], 1
    for n, tempered in lengths:
        pieces.append((g, g + n - 1, tempered, form_of(g, g + n - 1, tempered, k)))
        g += n
    return pieces


def schedule(short_rounds=2):
    """[(g_from, g_to, tempered, form)], tiling 1..G.  Two long pieces across five boundaries each, plain and tempered, each behind
    a piece shorter than K, each starting inside a window and ending with one; then pieces inside one window: whole windows and windows
    cut 2 + 3 (plain) and 3 + 2 (tempered).  short_rounds = 2: 3 + 27 + 2 + 28 + 40 = 100 generations, at least 22 per form."""
    lengths = [(3, False), (27, False), (2, True), (28, True)]
    lengths += [(5, False), (5, True)] * 2
    lengths += [(2, False), (3, False), (3, True), (2, True)] * short_rounds
    return pieces_of(lengths)


def temperatures(G, hot=10.0, cold=0.25):
    """Hot and cold generations in turn, never near 1: a kernel that ignored the temperature, or took a neighbouring generation's,
    accepts differently in every piece."""
    g = np.arange(1, G + 1)
    return np.where(g % 2 == 1, hot, cold) * (1.0 + 0.1 * np.sin(g))


# ---- block structures ---------------------------------------------------------------------------------------------------------------
def grouped(d, blocks, kind="mvn"):
    """demcz_create's rule: an MvNormal target whose blocks, in order, are consecutive index ranges covering 0..d-1 (any order inside
    a block) has the sums of its quadratic form cut at the block boundaries."""
    if kind != "mvn" or len(blocks) < 2 or sum(len(b) for b in blocks) != d:
        return False
    lo = 0
    for b in blocks:
        if sorted(b) != _r(lo, lo + len(b)):
            return False
        lo += len(b)
    return True


def incremental(d, blocks, env=()):
    return d == 20 and [list(b) for b in blocks] == [_r(0, 5), _r(5, 10), _r(10, 15), _r(15, 20)] and "DEMCZ_NO_MLB_INCREMENTAL" not in env


FOUR_BY_FIVE = [_r(0, 5), _r(5, 10), _r(10, 15), _r(15, 20)]
# id -> (d, blocks, N, environment switches, gamma).  The jumps: the workload's 2.38 accepts 7 % of the block-steps and leaves most
# outcomes of a generation unseen; at these a chain moves in 0.5 to 0.9 of the generations (0.97 with five single-parameter blocks)
# and every outcome vector is seen (tests/test_block_cases.py holds each world to that).
MLB_WORLDS = {
    "d5_gm": (5, [[0, 1], [2, 3, 4]], N_MAIN, (), 0.6),
    "d5_singles": (5, [[3], [0], [4], [1], [2]], N_MAIN, (), 0.35),
    "d6_gm_permuted": (6, [[0], [1, 2], [5, 3, 4]], N_MAIN, (), 0.5),
    "d6_interleaved": (6, [[0, 2, 4], [1, 3, 5]], N_MAIN, (), 0.5),
    "d10_halves": (10, [_r(0, 5), _r(5, 10)], N_MAIN, (), 0.4),
    "d10_four": (10, [[0, 1], [2, 3], [4, 5], [6, 7, 8, 9]], 64, (), 0.35),
    "d10_interleaved": (10, [[9, 0], [1, 8, 2], [3, 4, 5, 6, 7]], N_MAIN, (), 0.4),
    "d20_4x5": (20, FOUR_BY_FIVE, N_MAIN, (), 0.25),
    "d20_4x5_full_evaluation": (20, FOUR_BY_FIVE, N_MAIN, ("DEMCZ_NO_MLB_INCREMENTAL",), 0.25),
    "d20_8_12": (20, [_r(0, 8), _r(8, 20)], N_MAIN, (), 0.25),
    "d20_10_3_7": (20, [_r(0, 10), _r(10, 13), _r(13, 20)], N_MAIN, (), 0.25),
    "d20_odd_even": (20, [_r(0, 20)[0::2], _r(0, 20)[1::2]], N_MAIN, (), 0.25),
    "d20_overlap": (20, [_r(0, 20), _r(0, 5)], N_MAIN, (), 0.2),           # (the longest block a 16-lane step holds is 28 > d)
}
MLB_LANES = {5: 8, 6: 8, 10: 8, 20: 16}
L32_WORLDS = tuple(w for w in MLB_WORLDS if w.startswith("d20"))

# one lane per chain: id -> (kind, d, blocks, gamma)
ONE_LANE_WORLDS = {
    # window_kernel<MVNORMAL, D, false>: consecutive blocks (grouped) and interleaved ones
    "mvn2_consecutive": ("mvn", 2, [[0], [1]], 0.9), "mvn2_swapped": ("mvn", 2, [[1], [0]], 0.9),
    "mvn3_consecutive": ("mvn", 3, [[0], [1, 2]], 0.8), "mvn3_interleaved": ("mvn", 3, [[0, 2], [1]], 0.8),
    "mvn4_consecutive": ("mvn", 4, [[0, 1], [2, 3]], 0.7), "mvn4_interleaved": ("mvn", 4, [[0, 2], [1, 3]], 0.7),
    "mvn5_consecutive": ("mvn", 5, [[0, 1], [2, 3, 4]], 0.6), "mvn5_interleaved": ("mvn", 5, [[0, 2, 4], [1, 3]], 0.6),
    "mvn8_consecutive": ("mvn", 8, [_r(0, 4), _r(4, 8)], 0.45), "mvn8_interleaved": ("mvn", 8, [_r(0, 8)[0::2], _r(0, 8)[1::2]], 0.45),
    "mvn10_consecutive": ("mvn", 10, [_r(0, 3), _r(3, 6), _r(6, 10)], 0.45), "mvn10_interleaved": ("mvn", 10, [_r(0, 10)[0::2], _r(0, 10)[1::2]], 0.4),
    "mvn20_consecutive": ("mvn", 20, FOUR_BY_FIVE, 0.25), "mvn20_interleaved": ("mvn", 20, [_r(0, 20)[0::2], _r(0, 20)[1::2]], 0.25),
    # window_kernel_generic<MVNORMAL>: grouped through goff
    "mvn7_consecutive": ("mvn", 7, [_r(0, 3), _r(3, 7)], 0.5), "mvn13_consecutive": ("mvn", 13, [_r(0, 6), _r(6, 13)], 0.35),
    "mvn13_interleaved": ("mvn", 13, [_r(0, 13)[0::2], _r(0, 13)[1::2]], 0.35),
    "mvn64_last_alone": ("mvn", 64, [_r(0, 63), [63]], 0.1),                # (bit 63 of the group-start mask)
    "mvn64_interleaved": ("mvn", 64, [_r(0, 64)[0::2], _r(0, 64)[1::2]], 0.12),
    "iso10": ("iso", 10, [_r(0, 3), _r(3, 6), _r(6, 10)], 1.2), "iso7": ("iso", 7, [[0, 2, 4, 6], [1, 3, 5]], 1.2),
    "lr10": ("lr", 10, [_r(0, 5), _r(5, 10)], 0.5), "lr26": ("lr", 26, [_r(0, 9), _r(9, 18), _r(18, 26)], 0.3),
    "lr7": ("lr", 7, [[0, 2, 4, 6], [1, 3, 5]], 0.5),
    "program7": ("prog", 7, [[0, 1, 2], [3, 4, 5, 6]], 0.5),
}
LR_NOBS = 90
GENERIC_DIMS = {"mvn": (7, 13, 64), "iso": (7,), "lr": (7,)}
TARGET_NAME = {"mvn": "MVNORMAL", "iso": "ISO_QUAD", "lr": "LINREG_SSE", "prog": "4"}       # (TARGET_PROGRAM = 4, demcz_device.h)

# 65 blocks at d = 10 (overlapping pairs and singles): more than MLB_MAX_BLOCKS, so lanes_per_chain = 0 falls back to one lane
MANY_BLOCKS = [[i % 10, (i + 3) % 10] if i % 2 else [i % 10] for i in range(MLB_MAX_BLOCKS + 1)]


def _problem(kind, d, N):
    if kind == "mvn":
        return demc.workloads.mvnormal_problem(d, N)
    if kind == "iso":
        return demc.workloads.iso_quad_problem(d, N)
    if kind == "lr":
        return demc.workloads.linreg_problem(d, N, nobs=LR_NOBS)
    r = np.random.default_rng(100 + d)           # (the program world of tests/test_gpu_kernel_choice.py)
    return dict(target=demc.ProgramTarget(ROSENBROCK, d), Zinit=np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N), d)) + 0.5),
                eps_scale=1e-3 * np.ones(d), closure=rosenbrock_closure)


# Hot and cold temperatures of the tempered pieces.  Where the log-density is steep against the jump (the regression targets, d = 64)
# a proposal is accepted or rejected almost whatever a temperature of 10 does to the difference: those worlds take 1000.
HOT_COLD = {("lr", 7): (1000.0, 0.25), ("lr", 10): (1000.0, 0.25), ("lr", 26): (1000.0, 0.25), ("mvn", 64): (1000.0, 0.25)}


def _seed(name):
    return 20261019 + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100000


def _case(name, kind, d, blocks, N, gamma, pieces, env=(), temperature=None, k=K, problem=None):
    """(problem: a world of another shape than _problem's -- tests/full_update_cases.py: other observation counts)"""
    G = pieces[-1][1]
    return dict(name=name, kind=kind, d=d, blocks=[list(b) for b in blocks], N=N, K=k, seed=_seed(name), gamma=gamma, env=tuple(env),
                problem=_problem(kind, d, N) if problem is None else problem, pieces=pieces, G=G, temperature=temperatures(G, *HOT_COLD.get((kind, d), (10.0, 0.25))) if temperature is None else temperature)


def mlb_case(name):
    d, blocks, N, env, gamma = MLB_WORLDS[name]
    return _case(name, "mvn", d, blocks, N, gamma, schedule(4 if name == "d5_singles" else 2), env)


def one_lane_case(name):
    kind, d, blocks, gamma = ONE_LANE_WORLDS[name]
    return _case(name, kind, d, blocks, N_MAIN, gamma, schedule())


def many_blocks_case():
    return _case("d10_65_blocks", "mvn", 10, MANY_BLOCKS, N_MAIN, 0.3, schedule())


# ---- four-wave workgroups of the split layout -----------------------------------------------------------------------------------------
# The library takes four-wave workgroups when ceil(N L / 64) >= 4 CUs (demcz_create: wpw).  N = 4 CUs (64 / L) + 5 (L = 8) or + 3
# (L = 16) leaves the last of 4 CUs / 4 + 1 workgroups partly filled.  Whether such a handle goes LIVE is the device's matter
# (live_wg_capacity: the workgroups of the LIVE kernel that fit a CU, times the CUs, halved): on the MI355X the d = 5 and d = 6
# kernels do, the d = 10 and d = 20 ones hold one workgroup per CU and run one launch per K-window.  So those three structures
# have a second world of N = 4 CUs (64 / L) - 5 or - 3: the same inequality, one workgroup per CU, the last one partly filled,
# and LIVE where two workgroups of the LIVE kernel fit a CU (what C3 runs at N = 4096): the d = 10 and the ungrouped d = 20 kernel;
# the d = 20 kernel with the group-start mask fits once and stays at one launch per K-window.  FOUR_WAVE_LIVE: the worlds that must
# go LIVE on the MI355X; the others are held to whichever of the two plans the handle's LIVE status names.
# 2K + 3 generations: a piece inside a window, then one across two boundaries.
FOUR_WAVE_WORLDS = (("d5_gm", 1), ("d6_interleaved", 1), ("d10_halves", 1), ("d20_8_12", 1), ("d20_odd_even", 1),
                    ("d10_halves", -1), ("d20_8_12", -1), ("d20_odd_even", -1))


FOUR_WAVE_LIVE = (("d5_gm", 1), ("d6_interleaved", 1), ("d10_halves", -1), ("d20_odd_even", -1))


def four_wave_population(d, cus, sign=1):
    return 4 * cus * 8 + 5 * sign if MLB_LANES[d] == 8 else 4 * cus * 4 + 3 * sign


def four_wave_case(name, sign=1, cus=MI355X_CUS):
    d, blocks, _, env, gamma = MLB_WORLDS[name]
    return _case("four_wave_%s_%s" % (name, "over" if sign > 0 else "under"), "mvn", d, blocks, four_wave_population(d, cus, sign), gamma,
                 pieces_of([(3, True), (2 * K, False)]), env)


def chain_waves(case):
    return (case["N"] * MLB_LANES[case["d"]] + 63) // 64


def per_window_launches(pieces, k=K):
    """The count of window launches behind every piece of a handle that launches once per K-window."""
    out, n = [], 0
    for a, b, _, _ in pieces:
        n += (b - 1) // k - (a - 1) // k + 1
        out.append(n)
    return out


# ---- named edges ----------------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = [(3, False), (9, False), (2, True), (11, True)]            # every form, 25 generations
TINY = [("d5_gm", N) for N in (1, 3, 5, 9)] + [("d20_4x5", N) for N in (1, 3, 5)]      # idle chain groups in the wave
ZERO_TEMPERATURE_WORLDS = ("d10_four", "d20_4x5")                                        # one per L, each on both layouts
NO_HISTORY_WORLDS = ("d10_halves", "d20_4x5")
LEFT_OUT = (5, [[0, 1], [3]])                                                            # parameters 2 and 4 are in no block
RESUMED_WORLDS = ("d20_4x5", "d6_gm_permuted")
RESUME_AT = 12                                                                           # (inside a window and inside a LIVE piece's range)


def edge_case(name, N=None, lengths=EDGE_LENGTHS, temperature=None, blocks=None, tag="edge"):
    d, b, n, env, gamma = MLB_WORLDS[name]
    return _case("%s_%s_N%d" % (tag, name, N or n), "mvn", d, b if blocks is None else blocks, N or n, gamma, pieces_of(lengths), env, temperature)


def zero_temperature_case(name):
    from small_wave_cases import temps_with_zeros
    return edge_case(name, lengths=[(3, True), (27, True), (5, True), (2, True), (3, True)], temperature=temps_with_zeros(40), tag="zero_temperature")


def left_out_case():
    return edge_case("d5_gm", blocks=LEFT_OUT[1], tag="left_out")


def resumed_case(name):
    """Two parts of one run: the handle is given its own state back (set_state) behind generation RESUME_AT, in the middle of a
    window; a short piece follows, then LIVE ones."""
    return edge_case(name, lengths=[(3, False), (RESUME_AT - 3, False), (3, False), (12, False), (2, True), (11, True)], tag="resumed")


# ---- kernel names -----------------------------------------------------------------------------------------------------------------------
def instantiation(case, layout, form, lanes=None):
    """The template arguments <D, L, REC, LIVE, QB, GM> of the window_kernel_mlb a piece runs; layout: "fused", "split"."""
    d, L = case["d"], lanes or MLB_LANES[case["d"]]
    rec, live = layout == "split", layout == "split" and form.startswith("LIVE")
    qb = 5 if L == 16 and incremental(d, case["blocks"], case["env"]) else 0
    return (d, L, rec, live, qb, qb == 0 and grouped(d, case["blocks"]))


def reported_name(inst):
    """What demcz_debug_kernel_name says of an instantiation (GM left out; the fused forms without any trailing argument)."""
    d, L, rec, live, qb, _ = inst
    if not rec:
        return "demcz::window_kernel_mlb<MVNORMAL, %d, %d>" % (d, L)
    return "demcz::window_kernel_mlb<MVNORMAL, %d, %d, true, %s%s>" % (d, L, "true" if live else "false", ", 5" if qb else "")


def one_lane_name(kind, d):
    """(A dimension without a specialisation launches window_kernel_generic<TARGET> and is reported under this name all the same:
    demcz_debug_kernel_name's known misreport.)"""
    return "demcz::window_kernel<%s, %d, false>%s" % (TARGET_NAME[kind], d, " (program)" if kind == "prog" else "")


def one_lane_specialised(kind, d):
    return d in {"mvn": (2, 3, 4, 5, 8, 10, 20), "iso": (10,), "lr": (10, 26), "prog": ()}[kind]


def instantiations_planned():
    """Every (instantiation, reported name) of window_kernel_mlb the GPU tests assert, 32-lane forms included."""
    out = set()
    for name in MLB_WORLDS:
        case = mlb_case(name)
        for layout in ("fused", "split"):
            out |= {instantiation(case, layout, p[3]) for p in case["pieces"]}
        if name in L32_WORLDS:
            out |= {instantiation(case, "split", p[3], lanes=32) for p in case["pieces"]}
    return out


def kernel_names_planned():
    names = {reported_name(i) for i in instantiations_planned()}
    return names | {one_lane_name(k, d) for k, d, _, _ in ONE_LANE_WORLDS.values()}


# ---- the oracle's runs ------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _oracle_pieces(O, case, pieces, X, lp, Z, M, tempered=True):
    """The oracle over `pieces` from the state given (changed in place).  tempered = False: the same pieces without temperatures."""
    w, N, d = case["problem"], case["N"], case["d"]
    a0, G = pieces[0][0], pieces[-1][1] - pieces[0][0] + 1
    if case["kind"] == "prog":
        # (a temperature of exactly 1 divides exactly: the plain pieces of the Python loop)
        T = np.ones(G)
        for a, b, t, _ in pieces:
            if t and tempered:
                T[a - a0:b - a0 + 1] = case["temperature"][a - 1:b]
        r = oracle_sample_logobj(O, w["closure"], Z[:M], N, case["K"], G, case["blocks"], w["eps_scale"], case["gamma"], case["seed"],
                                 temperature=T, X0=X, lp0=lp, g_from=a0)
        return dict(chain=r["chain"], log_obj=r["log_obj"], changed=r["changed"], X=r["X"], logp=r["logp"], Z=r["Z"], M=r["M"])
    prob = O.Problem(N, d, case["K"], Z.shape[0], w["eps_scale"], case["seed"], blocks=case["blocks"], target=w["target"].spec())
    chain, lobj, changed = np.zeros((N, d, G), order="F"), np.zeros((N, G), order="F"), np.zeros(G, dtype=np.int64)
    for a, b, t, _ in pieces:
        M, ch, lo, cg = O.run(prob, X, lp, Z, M, a, b, case["gamma"], temperature=case["temperature"][a - 1:b] if t and tempered else None)
        chain[:, :, a - a0:b - a0 + 1], lobj[:, a - a0:b - a0 + 1], changed[a - a0:b - a0 + 1] = ch, lo, cg
    return dict(chain=chain, log_obj=lobj, changed=changed, X=X, logp=lp, Z=Z[:M].copy(), M=M)


def _start(O, case):
    w, N, d, G = case["problem"], case["N"], case["d"], case["G"]
    Z0 = w["Zinit"]
    M0 = Z0.shape[0]
    Z = np.zeros((M0 + N * (G // case["K"] + 1), d), order="F")
    Z[:M0] = Z0
    X = np.array(Z0[M0 - N:], order="F")
    if case["kind"] == "prog":
        lp = np.array([np.float64(w["closure"]([float(v) for v in X[c]])) for c in range(N)])
    else:
        lp = O.logp(O.Problem(N, d, case["K"], Z.shape[0], w["eps_scale"], case["seed"], blocks=case["blocks"], target=w["target"].spec()), X)
    return X, lp, Z, M0


def oracle_run(O, case):
    """The oracle over the case's pieces, computed once per world and left unchanged.  dict(chain, log_obj, X, logp, Z, M, changed,
    X0, lp0)."""
    if case["name"] not in _RUNS:
        X, lp, Z, M = _start(O, case)
        X0, lp0 = X.copy(), lp.copy()
        r = _oracle_pieces(O, case, case["pieces"], X, lp, Z, M)
        r.update(X0=X0, lp0=lp0)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[case["name"]] = r
    return _RUNS[case["name"]]


def untempered_differences(O, case, ref):
    """Per tempered piece: the number of chains whose history inside the piece differs when the oracle is started again at the
    piece's start from the reference's state there and runs the piece WITHOUT its temperatures."""
    N, K, out = case["N"], case["K"], []
    M0 = case["problem"]["Zinit"].shape[0]
    for a, b, tempered, _ in case["pieces"]:
        if not tempered:
            continue
        X = np.array(ref["chain"][:, :, a - 2] if a > 1 else ref["X0"], order="F")
        lp = np.array(ref["log_obj"][:, a - 2] if a > 1 else ref["lp0"])
        M = M0 + N * ((a - 1) // K)
        Z = np.zeros((M + N * ((b - a) // K + 2), case["d"]), order="F")
        Z[:M] = ref["Z"][:M]
        r = _oracle_pieces(O, case, [(a, b, True, "")], X, lp, Z, M, tempered=False)
        out.append(int((r["chain"] != ref["chain"][:, :, a - 1:b]).any(axis=(1, 2)).sum()))
    return out


def block_outcomes(case, ref):
    """moved[c, g - 1, ib]: a parameter of block ib differs between generations g - 1 and g of chain c (disjoint blocks and a
    positive eps: an accepted block-step moves every parameter of its block)."""
    full = np.concatenate([ref["X0"][:, :, None], ref["chain"]], axis=2)
    diff = full[:, :, 1:] != full[:, :, :-1]
    return np.stack([diff[:, b, :].any(axis=1) for b in case["blocks"]], axis=2)


def outcome_counts(case, ref):
    """{form: counts[2 ** NB]} of the outcome vectors of a generation (block 0 the highest bit) over the form's pieces."""
    moved = block_outcomes(case, ref)
    NB = len(case["blocks"])
    code = (moved * (1 << np.arange(NB - 1, -1, -1))).sum(axis=2)
    counts = {f: np.zeros(1 << NB, dtype=np.int64) for f in FORMS}
    for a, b, _, form in case["pieces"]:
        counts[form] += np.bincount(code[:, a - 1:b].ravel(), minlength=1 << NB)
    return counts


def pair_counts(case, ref):
    """{form: counts[NB, 2, 2]} of (the block-step before's outcome, this one's), the wrap from a generation's last block to block 0
    of the next included (the form is that of the later block-step's piece)."""
    moved = block_outcomes(case, ref)
    N, G, NB = moved.shape
    flat = moved.reshape(N, G * NB)
    counts = {f: np.zeros((NB, 2, 2), dtype=np.int64) for f in FORMS}
    for a, b, _, form in case["pieces"]:
        for s in range(max((a - 1) * NB, 1), b * NB):
            for p in (0, 1):
                for q in (0, 1):
                    counts[form][s % NB, p, q] += int(((flat[:, s - 1] == p) & (flat[:, s] == q)).sum())
    return counts


def disjoint(case):
    flat = [i for b in case["blocks"] for i in b]
    return len(flat) == len(set(flat))
