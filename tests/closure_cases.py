"""The worlds and schedules of the host-closure tests (no GPU, no assertions).

The host-closure mode (demcz_capi.hip: propose_kernel, accept_commit_kernel, end_generation_kernel behind demcz_propose,
demcz_closure_buffers, demcz_accept_commit, demcz_end_generation) takes d and the block table at run time, so one kernel serves
every shape; what differs between worlds is the block structure, the dimension, the population and the call protocol:
  * "copies": demcz_propose copies the proposals out, demcz_accept_commit copies the values in;
  * "pinned": demcz_closure_buffers -- the kernel stores the proposals to host memory, the last workgroup raises the flag the
    host spins on, the commit is only enqueued;
  * "pinned-own-pointers": the pinned buffers with the caller's own arrays passed all the same.
An oracle run does not depend on the layout, so a closure world IS a world of tests/block_cases.py or tests/full_update_cases.py
(its problem, gamma, seed, K = 5, population, schedule and temperatures; block_cases.oracle_run keeps the run by name), run
through the closure protocol with a batched closure that is the oracle's own log-density on a Problem with the world's blocks (the
sums are cut at block boundaries), rosenbrock_closure for program7.  A tempered piece passes
temperature[g - 1] to every demcz_accept_commit of generation g, a plain piece passes none.

Two references: block_cases.oracle_run (the oracle's own generation loop) and proposal_loop (helpers.oracle_sample_logobj around
the same closure: every proposal xprop[N, d, G, NB], accepted or not).  tests/test_closure_cases.py ties them together bit for bit
and holds the worlds to their conditions from the oracle alone; tests/test_gpu_closure_forms.py compares the library with both.

Conditions per main world, measured with the oracle (tests/test_closure_cases.py prints them; plain / tempered = the generations
of the plain / tempered pieces, LIVE and non-LIVE forms of block_cases summed): the rarest of the 2^NB block-outcome vectors
(disjoint blocks, NB <= 5) or of moved / did not move and the four (previous, this) pairs (one block) | the fewest chains a
tempered piece changes when it is run without its temperatures.  (d5_singles runs block_cases' 120 generations, left_out its 25.)
  world              d NB gamma  moved | plain tempered | chains      world              d NB gamma  moved | plain tempered | chains
  d5_gm              5  2 0.6    0.657 |   646     921 |  58          program7           7  2 0.5    0.637 |   638     967 |  52
  d5_singles         5  5 0.35   0.968 |   136      94 |  80          left_out           5  2 0.6    0.589 |   134     231 |  45
  d6_gm_permuted     6  3 0.5    0.785 |   277     442 |  66          many_blocks       10 65 0.3    1.000 |     -       - |  96
  d6_interleaved     6  2 0.5    0.653 |   685     976 |  49          full_mvn2          2  1 0.9    0.391 |   453     945 |  40
  d10_four          10  4 0.35   0.883 |    95     119 |  53          full_mvn3          3  1 0.7    0.383 |   523     858 |  31
  d10_interleaved   10  3 0.4    0.784 |   308     415 |  62          full_mvn5          5  1 0.45   0.438 |   714    1010 |  29
  d20_4x5           20  4 0.25   0.894 |   174     232 |  44          full_mvn7          7  1 0.35   0.435 |   801     995 |  11
  d20_10_3_7        20  3 0.25   0.829 |   407     493 |  34          full_mvn9          9  1 0.28   0.483 |   989    1076 |   9
  d20_odd_even      20  2 0.25   0.711 |   971    1148 |  17          full_mvn13        13  1 0.22   0.491 |  1020    1073 |  10
  d20_overlap       20  2 0.2    0.729 |     -       - |  20          full_mvn20        20  1 0.25   0.464 |  1000    1055 |   5
  mvn2_swapped       2  2 0.9    0.649 |   646    1017 |  55          full_mvn64        64  1 0.08   0.605 |  1164     150 |  41
  mvn3_interleaved   3  2 0.8    0.640 |   639     998 |  56          full_iso10        10  1 1.2    0.526 |  1045     519 |  48
  mvn13_interleaved 13  2 0.35   0.671 |   811    1039 |  23          full_lr26         26  1 0.3    0.576 |  1141     506 |  26
  mvn64_last_alone  64  2 0.1    0.775 |  1011     626 |  73          iso1               1  1 2.0    0.403 |   556     987 |  32
  mvn64_interleaved 64  2 0.12   0.789 |  1113     701 |  65          mvn33             33  1 0.14   0.490 |  1116    1188 |   3
  iso7               7  2 1.2    0.761 |  1123     821 |  64          (the two new worlds' rarest pair over block_cases' four
  lr10              10  2 0.5    0.732 |   929     676 |  66           forms: iso1 240, mvn33 483)
  lr7                7  2 0.5    0.715 |   878     683 |  76
Edge worlds: acceptance 0.810-0.827 at N = 63 ... 257, 18 moved / 7 not of 25 generations at N = 1, 0.645-0.776 in the other worlds
of d6_gm_permuted, 0.673 and 0.527 under T = 0 / 1e-300 / 1e300 (d = 6 blocks, d = 64); the box closure returns -inf 614, NaN 73
and +inf 32 times in 3200 proposals.
"""
import numpy as np

import demc_jl_amd as demc

import block_cases as bc
import full_update_cases as fc
from block_cases import K, N_MAIN, pieces_of, schedule
from helpers import oracle_sample, oracle_sample_logobj
from small_wave_cases import temps_with_zeros

MODES = ("copies", "pinned", "pinned-own-pointers")
EDGE_MODES = ("copies", "pinned")
PROPOSE_BS, COMMIT_BS = 64, 256          # WINDOW_BS lanes of propose_kernel / end_generation_kernel; accept_commit_kernel's 256

# ---- main worlds ------------------------------------------------------------------------------------------------------------------------
BLOCK_WORLDS = ("d5_gm", "d5_singles", "d6_gm_permuted", "d6_interleaved", "d10_four", "d10_interleaved", "d20_4x5", "d20_10_3_7",
                "d20_odd_even", "d20_overlap", "mvn2_swapped", "mvn3_interleaved", "mvn13_interleaved", "mvn64_last_alone",
                "mvn64_interleaved", "iso7", "lr10", "lr7", "program7", "left_out", "many_blocks")
FULL_WORLDS = ("mvn2", "mvn3", "mvn5", "mvn7", "mvn9", "mvn13", "mvn20", "mvn64", "iso10", "lr26")
# id -> (kind, d, gamma): found with the oracle alone so that a chain moves in 0.25 to 0.75 of its generations
NEW_WORLDS = {
    "iso1": ("iso", 1, 2.0),                   # b = 1 and d = 1 at once: scale = gamma, one normal
    "mvn33": ("mvn", 33, 0.14),                # an odd block above 32: 17 pairs, the last pair's second normal unused
}
MAIN_WORLDS = BLOCK_WORLDS + tuple("full_" + w for w in FULL_WORLDS) + tuple(NEW_WORLDS)


def _iso1_problem(N):
    w = demc.workloads.iso_quad_problem(1, N)
    w["target"], w["mu"] = demc.targets.IsoQuadTarget(np.zeros(1)), np.zeros(1)
    return w


def main_case(name):
    if name == "left_out":
        return bc.left_out_case()                     # (25 generations, every form: block_cases' own edge world)
    if name == "many_blocks":
        return bc.many_blocks_case()
    if name in bc.MLB_WORLDS:
        return bc.mlb_case(name)
    if name in bc.ONE_LANE_WORLDS:
        return bc.one_lane_case(name)
    if name.startswith("full_"):
        return fc.case_of(name[5:])
    kind, d, gamma = NEW_WORLDS[name]
    return bc._case("closure_" + name, kind, d, [list(range(d))], N_MAIN, gamma, schedule(), problem=_iso1_problem(N_MAIN) if name == "iso1" else None)


def one_block(case):
    return case["blocks"] == [list(range(case["d"]))]


# ---- the closures ----------------------------------------------------------------------------------------------------------------------
def batched_closure(O, case):
    """X (n x d) -> n log-densities: what the library is handed."""
    w = case["problem"]
    if case["kind"] == "prog":
        f = w["closure"]
        return lambda X: np.array([np.float64(f([float(v) for v in row])) for row in np.asarray(X)])
    prob = O.Problem(case["N"], case["d"], case["K"], 10, w["eps_scale"], 0, blocks=case["blocks"], target=w["target"].spec())
    return lambda X: O.logp(prob, np.asarray(X))


def row_closure(O, case):
    """A list of d Python floats -> the same closure's value: what helpers.oracle_sample_logobj calls."""
    if case["kind"] == "prog":
        return case["problem"]["closure"]
    f = batched_closure(O, case)
    return lambda x: f(np.array([x]))[0]


def piece_temperatures(case):
    """One temperature per generation for a loop that always divides: the tempered pieces' own, exactly 1 (which divides exactly)
    in the plain ones."""
    T = np.ones(case["G"])
    for a, b, tempered, _ in case["pieces"]:
        if tempered:
            T[a - 1:b] = case["temperature"][a - 1:b]
    return T


def temperature_of(case, g):
    """What demcz_accept_commit is passed in generation g: the temperature, or None in a plain piece."""
    for a, b, tempered, _ in case["pieces"]:
        if a <= g <= b:
            return float(case["temperature"][g - 1]) if tempered else None
    raise ValueError(g)


# ---- the references ----------------------------------------------------------------------------------------------------------------------
_LOOPS, _OFFSET_RUNS = {}, {}


def reference(O, case):
    """The oracle's run of the case (block_cases.oracle_run; a world with a Python closure: the loop below), or with a
    rng_offset the oracle's run at that offset."""
    if case.get("rng_offset"):
        if case["name"] not in _OFFSET_RUNS:
            w = case["problem"]
            r = oracle_sample(O, w["target"], w["Zinit"], case["N"], case["K"], case["G"], case["blocks"], w["eps_scale"], case["gamma"],
                              case["seed"], temperature=piece_temperatures(case), rng_offset=case["rng_offset"])
            _OFFSET_RUNS[case["name"]] = r
        return _OFFSET_RUNS[case["name"]]
    return bc.oracle_run(O, case)


def proposal_loop(O, case):
    """helpers.oracle_sample_logobj around the case's closure, once per world: its dict with `xprop` (N, d, G, NB), left
    unchanged.  N G NB calls of the oracle's block_step."""
    if case["name"] not in _LOOPS:
        w = case["problem"]
        r = oracle_sample_logobj(O, row_closure(O, case), w["Zinit"], case["N"], case["K"], case["G"], case["blocks"], w["eps_scale"],
                                 case["gamma"], case["seed"], temperature=piece_temperatures(case), with_xprop=True,
                                 rng_offset=case.get("rng_offset", 0))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _LOOPS[case["name"]] = r
    return _LOOPS[case["name"]]


def plain_tempered(counts):
    """block_cases.outcome_counts / pair_counts per form -> {"plain": ..., "tempered": ...}: LIVE and non-LIVE summed."""
    return {t: sum(c for f, c in counts.items() if f.endswith(t)) for t in ("plain", "tempered")}


# ---- edge worlds ---------------------------------------------------------------------------------------------------------------------------
EDGE_WORLD = "d6_gm_permuted"
POPULATIONS = (1, 63, 64, 65, 129, 255, 256, 257)
ALTERNATE = [(1, True), (1, False)] * 12 + [(1, True)]                # 25 generations, every generation tempered in turn
LENGTHS_40 = [(3, False), (17, False), (2, True), (18, True)]
LENGTHS_41 = LENGTHS_40 + [(1, False)]
LENGTHS_45 = LENGTHS_40 + [(5, False)]
ZERO_LENGTHS = fc.ZERO_LENGTHS                                        # 40 generations, all tempered
SWITCH_AT = 12                                                        # copies up to here, then demcz_closure_buffers
ORIGIN = 20
RNG_OFFSET = 7


def _edge(tag, N=None, lengths=bc.EDGE_LENGTHS, k=K, temperature=None, **extra):
    d, blocks, n, env, gamma = bc.MLB_WORLDS[EDGE_WORLD]
    N = n if N is None else N
    case = bc._case("closure_%s_N%d" % (tag, N), "mvn", d, blocks, N, gamma, pieces_of(lengths, k), env, temperature, k=k)
    case.update(extra)
    return case


def population_case(N):
    return _edge("population", N=N, lengths=ALTERNATE)


def workgroups(N):
    """(propose / end-generation workgroups, commit workgroups) of a population."""
    return -(-N // PROPOSE_BS), -(-N // COMMIT_BS)


def archive_case(k):
    """K = 1: an append after every generation; K = 41 > G = 40: none."""
    return _edge("K%d" % k, lengths=LENGTHS_40, k=k)


def capacity_case():
    """Mcap exactly the rows of 40 generations, then one more boundary generation (45): its append is refused."""
    return _edge("capacity", lengths=LENGTHS_45)


def no_history_case():
    return _edge("no_history", lengths=LENGTHS_40)


def origin_case():
    """Gcap = 20, the origin moved to 20 behind generation 20; generation 41 is outside the window."""
    return _edge("origin", lengths=LENGTHS_41)


def rng_offset_case():
    return _edge("rng_offset", lengths=LENGTHS_40, rng_offset=RNG_OFFSET)


def plain_edge_case():
    """N = 96, 25 generations, every form: the shards (two handles of 48), the one-rank communicator, the refusals."""
    return _edge("edge")


def switch_case():
    return _edge("switch", lengths=LENGTHS_40)


def zero_temperature_cases():
    """T = 0, 1e-300, 1e300 and 2.5 in turn, at d = 6 in blocks and at d = 64 in one block."""
    return [_edge("zero_temperature", lengths=ZERO_LENGTHS, temperature=temps_with_zeros(40)), fc.zero_temperature_case("mvn64")]


# A box closure at d = 4, blocks [[0, 1], [2, 3]]: the quadratic inside |x_i| <= BOX, -inf outside, NaN behind the face
# x_0 = +BOX, +inf in the small cube around one point (a single point is never proposed: the proposals are continuous).  A
# chain that reaches +inf stays there: (lp' - inf) is -inf or NaN.
BOX, PEAK, PEAK_HALF_WIDTH = 1.0, (0.25, -0.25, 0.25, -0.25), 0.2
BOX_BLOCKS = [[0, 1], [2, 3]]


def box_closure(x):
    if x[0] > BOX:
        return float("nan")
    if any(abs(v) > BOX for v in x):
        return -float("inf")
    if all(abs(v - p) <= PEAK_HALF_WIDTH for v, p in zip(x, PEAK)):
        return float("inf")
    s = 0.0
    for v in x:
        s = s + v * v
    return -0.5 * s


def box_case():
    N, d = 64, 4
    r = np.random.default_rng(20261021)
    Z = np.asfortranarray(r.uniform(-0.9, 0.9, size=(2 * N, d)))
    start = Z[-N:]
    inside_peak = (np.abs(start - np.array(PEAK)) <= PEAK_HALF_WIDTH).all(axis=1)
    start[inside_peak, 0] = -0.5                                   # (the start is inside the box and outside the cube)
    problem = dict(Zinit=Z, eps_scale=1e-3 * np.ones(d), closure=box_closure)
    return bc._case("closure_box", "prog", d, BOX_BLOCKS, N, 0.9, pieces_of(ALTERNATE), problem=problem)


def box_kinds(proposed):
    """(-inf, NaN, +inf) counts among the closure's values of every proposal."""
    return int(np.isneginf(proposed).sum()), int(np.isnan(proposed).sum()), int(np.isposinf(proposed).sum())


# ---- the sampler surface ---------------------------------------------------------------------------------------------------------------------
SURFACE = dict(d=6, N=24, K=5, G=30, blocks=[[0], [1, 2], [5, 3, 4]], gamma=0.5, seed=20261021)
PREVRUN = dict(d=20, N=48, K=5, G1=30, G2=35, seed=77, gamma=0.25,
               second=[list(range(0, 5)), list(range(5, 10)), list(range(10, 15)), list(range(15, 20))])


def edge_cases():
    """Every edge case that runs the closure protocol against a reference of its own (what the CPU tier holds to an acceptance)."""
    out = [population_case(N) for N in POPULATIONS] + [archive_case(1), archive_case(41), capacity_case(), no_history_case(), origin_case(),
                                                       rng_offset_case(), plain_edge_case(), switch_case()]
    return out + zero_temperature_cases() + [box_case()]

