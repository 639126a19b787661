"""The worlds, plans and counts of the replica-group tests (no GPU, no assertions).

A replica group (demcz_peer_group) is R handles of one process, each with 1 / R of the chains and a replica of the whole archive.
Every member's LIVE launches store a K boundary's rows into every replica (live_publish, demcz_kernels_rec.h); readers poll their
own replica.  Against a single handle three things change in every publishing site -- a boundary appends brows = N_total rows,
local chain cl lands at row_off + cl, and most rows a wave waits for are written by another launch -- and none of them shows on
a single handle (row_off = 0, brows = N, no peers).  Here: the worlds of the single-handle suites (small_wave_cases,
dimension_cases, block_cases, full_update_cases; their targets, schedules, seeds and oracle runs, kept by name) cut into R equal
shards: member r has chain_id0 = r n_loc, rows r n_loc .. (r + 1) n_loc - 1 of the starting population and the whole starting
archive; the oracle's UNSHARDED run at N_total is what every group is compared with.  tests/test_peer_cases.py checks the worlds
from the oracle alone, tests/test_gpu_peer_forms.py compares the library.

What a member of a group with the hand-off runs (demcz_run_plan.h, plan_launch with `peer`; demcz_capi.hip, window_kernel_of):
  * its launches are cut as a single split handle's are (full_update_cases.split_live_launches: a launch runs to its call's end
    unless draws of K generations or more, but fewer than the call is long, are at hand) -- `member_walk` below restates the rule
    with the launches themselves, tests/test_peer_cases.py holds it to split_live_launches and to the executable planner;
  * EVERY launch is of the LIVE kind, a boundary inside it or not (the rows of the boundary that ended the launch before may
    still be on their way from another member's publisher): a piece that a single handle runs in a non-LIVE form runs the LIVE
    instantiation on a member.  So at d > 5 a five-generation piece from a multiple of five is a REG launch (pw_regular asks
    for LIVE), and a member never runs window_kernel_ps2d (peer_no_dual);
  * the forms of a schedule keep their single-handle names here ("non-LIVE plain": a call inside one K-window) -- they are the
    shapes of the calls; `member_name` gives the kernel a member runs for each.
A group whose layout has no hand-off (one lane per chain, the fused 8 / 16-lane kernels, pc8) runs in lockstep from the start
(G->lockstep_only): its members only log their calls, and the next verification executes them for all members one launch per
K-window, the non-LIVE kernels, rows appended from the members' state buffers.
"""
import numpy as np

import demc_jl_amd as demc
import block_cases as bc
import dimension_cases as dc
import full_update_cases as fc
import small_wave_cases as sw
from helpers import SPLIT, SPLIT_WAVE

L32 = "DEMCZ_MLB_L32"                     # read once per process (demcz_capi.hip, mlb_l32)
SHAPE_N_LOC = ((1, 2), (3, 2), (5, 2), (9, 2), (17, 2), (7, 3))       # (n_loc, R): a last workgroup partly filled, or an only one mostly idle
ARCHIVE_EXTRA = 8                          # the small worlds' archive: the last N_total + 8 rows of the workload's Zinit
# every form of the K = 10 families in 50 generations, built as block_cases.EDGE_LENGTHS is: each long piece behind one shorter
# than K.  1..5 a pass inside a window; 6..15 and 16..25 regular across a boundary (the second served by the first's draws: as
# long as the call); 26..27, 28..33, 34..35, 36..43 general, inside a window and across a boundary, plain and tempered; 46..50 a
# tempered pass
K10_EDGE_LENGTHS = [(5, False), (10, False), (10, True), (2, False), (6, False), (2, True), (8, True), (2, True), (5, True)]
K10_ZERO_LENGTHS = [(5, True), (20, True), (3, True), (9, True), (3, True)]           # steady and general, inside a window and across
PW_MAIN_PIECES = 11                        # dimension_cases.pw_schedule()[:11]: 200 generations, six forms
PW_R3_DIMS, PW_ISO_DIMS = (6, 20, 32), (6, 10, 32)
PW_R3_POPULATION = 192
MLB_R3_WORLDS = ("d5_gm", "d20_4x5")

# seeds: the first of seed, seed + 1, ... at which the oracle's draws alone meet the conditions of tests/test_peer_cases.py (a main
# run: 8 hand-off steps per ordered pair of ranks and LIVE form -- the worlds listed have 5 to 7 somewhere at their module's seed;
# two chains in all: a hand-off in both directions at all).  A world not listed keeps its module's seed and its oracle run.
SEED_BUMP = {"ps d5 R3": 4, "pw mvn d8 R2": 1, "pw mvn d16 R2": 1, "pw mvn d20 R3": 1, "pw mvn d22 R2": 1, "pw mvn d23 R2": 1, "pw mvn d27 R2": 1,
             "pw mvn d28 R2": 1, "pw mvn d29 R2": 1, "pw mvn d31 R2": 1, "pw mvn d32 R3": 4, "ml mvn20 R3": 1, "lr16_obs1153 lr10_matrix R2": 4,
             "ps d3 2x1": 5, "ps d5 2x1": 4, "pw mvn d6 2x1": 5, "pw mvn d23 2x1": 3, "ml mvn20 2x1": 4}


# ---- a member's launches ----------------------------------------------------------------------------------------------------------------
def member_walk(pieces, k, cold_behind=()):
    """[[(g, w_end), ...] per piece]: the window launches of a member with the hand-off (a span longer than any piece, no hint of
    the next call), and per piece the generations of draws at hand when it starts.  cold_behind: generations behind which
    demcz_set_state has thrown the prepared draws away."""
    out, at_hand, prepared = [], [], 0
    for a, b, _, _ in pieces:
        at_hand.append(prepared)
        launches, g = [], a
        while g <= b:
            m = b - g + 1
            if k <= prepared < m:
                m = max(prepared // k * k, k)
            launches.append((g, g + m - 1))
            g += m
            prepared = b - g + 1 if g <= b else b - a + 1
        if b in cold_behind:
            prepared = 0
        out.append(launches)
    return out, at_hand


def lockstep_walk(pieces, k):
    """The launches of a lockstep group (group_execute): one per K-window of every call."""
    out = []
    for a, b, _, _ in pieces:
        launches, g = [], a
        while g <= b:
            e = min(((g - 1) // k + 1) * k, b)
            launches.append((g, e))
            g = e + 1
        out.append(launches)
    return out


def counts_behind(walk):
    return list(np.cumsum([len(launches) for launches in walk]).tolist())


# ---- kernel names ---------------------------------------------------------------------------------------------------------------------
def _live(form):
    """The form whose kernel a member runs for a call of `form`: the LIVE one."""
    return form.replace("non-LIVE", "LIVE")


def pw_member_form(a, b, tempered, k):
    """dimension_cases.form_of with `live` true whatever lies inside the launch."""
    reg = k % dc.PASS == 0 and (k - (a - 1) % k) % dc.PASS == 0 and (b - a + 1) % dc.PASS == 0
    if reg:
        return dc.REG_TEMPERED if tempered else dc.REG_PLAIN
    return dc.LIVE_TEMPERED if tempered else dc.LIVE_PLAIN


def member_name(run, piece):
    """What demcz_debug_kernel_name must say on every member behind `piece`."""
    case, family = run["case"], run["family"]
    a, b, tempered, form = piece
    member = dict(case, N=run["n_loc"])
    if not run["handoff"]:
        if family == "one":
            return bc.one_lane_name(case["kind"], case["d"])
        if family == "pc8":
            return sw.pc8_kernel_name(case["kind"], case["d"], "non-LIVE " + ("tempered" if tempered else "plain"))
        return fc.planned_name(member, "fused", form)
    if family == "ps":
        return sw.kernel_name(case["d"], _live(form))
    if family == "pw":
        return dc.pw_kernel_name(case["kind"], case["d"], pw_member_form(a, b, tempered, case["K"]))
    if family == "mlb":
        return bc.reported_name(bc.instantiation(case, "split", _live(form), lanes=32 if L32 in run["env"] else None))
    return fc.planned_name(member, "split", _live(form), run["env"])          # ml, lr


def plan(run):
    """[(kernel name, window launches behind the piece)] of every member, and the first generation of the last launch."""
    case = run["case"]
    if run["handoff"]:
        walk, _ = member_walk(case["pieces"], case["K"], (run["resume_at"],) if run["resume_at"] else ())
    else:
        walk = lockstep_walk(case["pieces"], case["K"])
    return [(member_name(run, p), c) for p, c in zip(case["pieces"], counts_behind(walk))], walk[-1][-1][0]


# ---- worlds -----------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _kept(key, make):
    if key not in _REFS:
        r = make()
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _ref_of(case):
    """The oracle's unsharded run of the world, computed once and left unchanged.  block_cases keeps its runs by name (those of
    full_update_cases with them); dimension_cases.oracle_run keeps nothing, so the K = 10 worlds' runs are kept here."""
    if "name" in case:
        return lambda O: bc.oracle_run(O, case)
    key = (case["kind"], case["d"], case["N"], case["G"], case["seed"], case["problem"]["Zinit"].shape[0], tuple(case["pieces"]))
    return lambda O: _kept(key, lambda: dc.oracle_run(O, case))


def small_archive(case):
    """The world with the last N + ARCHIVE_EXTRA rows of its Zinit as its archive (its last N rows: the starting population, as
    before), under a name of its own."""
    Z = case["problem"]["Zinit"]
    w = dict(case["problem"], Zinit=np.asfortranarray(Z[-min(Z.shape[0], case["N"] + ARCHIVE_EXTRA):]))
    out = dict(case, problem=w)
    if "name" in case:
        out["name"] = case["name"] + "_archive%d" % w["Zinit"].shape[0]
    return out


def pw_edge_case(kind, d, N, lengths, temperature=None):
    """dimension_cases.pw_case at another population and schedule."""
    w = (demc.workloads.mvnormal_problem if kind == "mvn" else demc.workloads.iso_quad_problem)(d, N)
    pieces = sw._pieces(lengths, dc.form_of)
    G = pieces[-1][1]
    return dict(kind=kind, d=d, N=N, K=dc.K, seed=20261019 + 100 * d + 7 * N + (kind == "iso"), gamma=dc.PW_GAMMA[kind], problem=w,
                pieces=pieces, G=G, temperature=dc.temperatures(G) if temperature is None else temperature)


def pw_main_case(kind, d, R=2):
    """dimension_cases.pw_case on the first eleven pieces of its schedule.  R = 3: at 192 chains -- with 3 x 32 the late general
    LIVE pieces (the archive then holds 1100 to 1900 rows) give an ordered pair of ranks 6 hand-off steps on average, and no seed
    gives all six pairs 8 in every form; 3 x 64 chains give 12."""
    case = dc.pw_case(kind, d)
    pieces = case["pieces"][:PW_MAIN_PIECES]
    if R == 3:
        return pw_edge_case(kind, d, PW_R3_POPULATION, [(b - a + 1, t) for a, b, t, _ in pieces])
    return dict(case, pieces=pieces, G=pieces[-1][1])


FAMILY_FORMS = {"ps": sw.ONE_FORMS, "pw": dc.FORMS, "mlb": bc.FORMS, "ml": bc.FORMS, "lr": bc.FORMS}
FAMILY_LANES = {"ps": (SPLIT_WAVE, SPLIT_WAVE), "pw": (SPLIT_WAVE, SPLIT_WAVE), "mlb": (SPLIT, SPLIT), "ml": (SPLIT, SPLIT), "lr": (SPLIT, SPLIT),
                "pc8": (SPLIT, SPLIT), "one": (1, 1)}


def _run(rid, kind, family, case, R, env=(), handoff=True, history=True, resume_at=None, lanes=None):
    """One group run.  lanes: (lanes_per_chain asked for, what the handle reports), where the family's are not meant."""
    bump = SEED_BUMP.get(rid, 0)
    if bump:
        case = dict(case, seed=case["seed"] + bump)
        if "name" in case:
            case["name"] += "_seed%d" % bump
    if case["N"] % R:
        raise ValueError("%s: %d chains in %d shards" % (rid, case["N"], R))
    if "blocks" not in case:
        case = dict(case, blocks=[list(range(case["d"]))])
    asked, reported = lanes or FAMILY_LANES[family]
    return dict(id=rid, kind=kind, family=family, case=case, R=R, n_loc=case["N"] // R, env=tuple(env), handoff=handoff, history=history,
                resume_at=resume_at, lanes=asked, layout=reported, ref=_ref_of(case))


def _lr_runs(kind, make, tag, R=2):
    """The regression world's three split members: lr8s; lr16 behind DEMCZ_NO_LR_SPEC; lr16 at one observation more than lr8s holds."""
    return [_run("lr8s %s R%d" % (tag, R), kind, "lr", make(None), R),
            _run("lr16_no_spec %s R%d" % (tag, R), kind, "lr", make(None), R, env=(fc.NO_LR_SPEC,)),
            _run("lr16_obs%d %s R%d" % (fc.LR8S_MAX_OBS + 1, tag, R), kind, "lr", make(fc.LR8S_MAX_OBS + 1), R)]


def main_runs():
    """R equal shards of the single-handle suites' main worlds, every form of the family on each member."""
    runs = []
    for d in sw.DIMS:
        for R in (2, 3) if d == 5 else (2,):
            runs.append(_run("ps d%d R%d" % (d, R), "main", "ps", sw.small_case(d, False), R))
    for kind, dims in (("mvn", dc.PW_DIMS), ("iso", PW_ISO_DIMS)):
        for d in dims:
            for R in (2, 3) if kind == "mvn" and d in PW_R3_DIMS else (2,):
                runs.append(_run("pw %s d%d R%d" % (kind, d, R), "main", "pw", pw_main_case(kind, d, R), R))
    for name in bc.MLB_WORLDS:
        for R in (2, 3) if name in MLB_R3_WORLDS else (2,):
            case = bc.mlb_case(name)
            runs.append(_run("mlb %s R%d" % (name, R), "main", "mlb", case, R, env=case["env"]))
    for R in (2, 3):
        case = fc.case_of("mvn20")
        runs.append(_run("ml mvn20 R%d" % R, "main", "ml", case, R))

    def lr_main(nobs):
        return fc.case_of(fc.LR_WORLD) if nobs is None else fc.case_of(fc.LR_WORLD, nobs=nobs, tag="main")
    return runs + _lr_runs("main", lr_main, "lr10_matrix")


def l32_run():
    """d20_4x5 once more on 32 lanes per chain: collected only in a process that has the switch."""
    case = bc.mlb_case("d20_4x5")
    return _run("mlb d20_4x5 L32 R2", "main", "mlb", case, 2, env=(L32,), lanes=(0, SPLIT))


def shape_runs():
    """One world per publishing site at (n_loc, R) of SHAPE_N_LOC, the small archive: fresh rows are a large share of every draw."""
    runs = []
    for n_loc, R in SHAPE_N_LOC:
        N, tag = n_loc * R, "%dx%d" % (R, n_loc)
        for d in (3, 5):                                         # (both run window_kernel_ps and window_kernel_ps2: the schedule has both)
            runs.append(_run("ps d%d %s" % (d, tag), "shape", "ps", small_archive(sw.edge_case(d, N, False, K10_EDGE_LENGTHS)), R))
        for d in (6, 23):
            runs.append(_run("pw mvn d%d %s" % (d, tag), "shape", "pw", small_archive(pw_edge_case("mvn", d, N, K10_EDGE_LENGTHS)), R))
        for name in ("d5_gm", "d20_4x5"):
            case = small_archive(bc.edge_case(name, N=N))
            runs.append(_run("mlb %s %s" % (name, tag), "shape", "mlb", case, R))
        case = small_archive(fc.edge_case("mvn20", N))
        runs.append(_run("ml mvn20 %s" % tag, "shape", "ml", case, R))
        case = small_archive(fc.lr_case(N=N))
        runs.append(_run("lr8s %s" % tag, "shape", "lr", case, R))
        runs.append(_run("lr16_no_spec %s" % tag, "shape", "lr", case, R, env=(fc.NO_LR_SPEC,)))
    return runs


def lockstep_runs():
    """Layouts without the hand-off: one lane per chain (in blocks: a grouped MvNormal and a program), the fused 8- and 16-lane
    kernels, the fused regression kernel, pc8.  R = 2, 25 generations with every form."""
    runs = []
    for name in ("mvn5_consecutive", "program7"):
        kind, d, blocks, gamma = bc.ONE_LANE_WORLDS[name]
        case = bc._case("edge_one_lane_" + name, kind, d, blocks, bc.N_MAIN, gamma, bc.pieces_of(bc.EDGE_LENGTHS))
        runs.append(_run("one %s" % name, "lockstep", "one", case, 2, handoff=False))
    for name in ("mvn8", "mvn20", fc.LR_WORLD):
        case = fc.edge_case(name)
        runs.append(_run("fused %s" % name, "lockstep", "fused", case, 2, handoff=False, lanes=(fc.lanes_of(case),) * 2))
    for name in ("mvn5", "iso10"):
        case = fc.edge_case(name)
        runs.append(_run("pc8 %s" % name, "lockstep", "pc8", case, 2, handoff=False))
    return runs


def edge_runs():
    """Gcap = 0; a group given its own state back in the middle of a window; zero, tiny and huge temperatures."""
    runs = [_run("no_history pw mvn d6", "edge", "pw", pw_edge_case("mvn", 6, 96, K10_EDGE_LENGTHS), 2, history=False)]
    case = bc.edge_case("d5_gm")
    runs.append(_run("no_history mlb d5_gm", "edge", "mlb", case, 2, history=False))
    runs.append(_run("resumed ps d5", "edge", "ps", sw.edge_case(5, 96, False, fc.RESUMED_LENGTHS), 2, resume_at=fc.RESUME_AT))
    case = fc.resumed_case("mvn20")
    runs.append(_run("resumed ml mvn20", "edge", "ml", case, 2, resume_at=fc.RESUME_AT))
    runs.append(_run("zero_temperature ps2 d4", "edge", "ps", sw.edge_case(4, 96, False, K10_ZERO_LENGTHS, temperature=sw.temps_with_zeros(40)), 2))
    case = bc.zero_temperature_case("d20_4x5")
    runs.append(_run("zero_temperature mlb d20_4x5", "edge", "mlb", case, 2))
    return runs


def all_runs():
    return main_runs() + [l32_run()] + shape_runs() + lockstep_runs() + edge_runs()


def ids(runs):
    return [r["id"].replace(" ", "-") for r in runs]


def kernel_names_planned(runs=None):
    """Every kernel name the group tests assert."""
    return {name for r in (all_runs() if runs is None else runs) for name, _ in plan(r)[0]}


# ---- what the oracle's draws say of a run ------------------------------------------------------------------------------------------------
ACROSS_CALLS = "across calls"


def _steps(case):
    """(blocks of the Philox stream per generation, the offset of every block-step's first block): the oracle's numbering."""
    offs, s = [], 0
    for b in case["blocks"]:
        offs.append(s)
        s += 1 + (len(b) + 1) // 2 + 1
    return s, offs


def _form_at(case, g):
    """The form of the piece that holds generations g and g + 1, or ACROSS_CALLS."""
    for a, b, _, form in case["pieces"]:
        if a <= g < b:
            return form
    return ACROSS_CALLS


def handoff_counts(O, case, R):
    """{(reader rank, writer rank, form): block-steps}: the steps of generation bK + 1 that draw a row appended at boundary b, over
    every boundary of the run with a generation behind it; form: of the piece that holds both generations (ACROSS_CALLS where bK
    ends a call: the rows are then handed from one launch to the next)."""
    N, K, G = case["N"], case["K"], case["G"]
    n_loc, M0 = N // R, case["problem"]["Zinit"].shape[0]
    S, offs = _steps(case)
    counts = {}
    for b in range(1, (G - 1) // K + 1):
        g, M = b * K + 1, M0 + b * N
        form = _form_at(case, b * K)
        for c in range(N):
            for off in offs:
                fresh = {(i - (M - N)) // n_loc for i in O.draw_rows(case["seed"], c, (g - 1) * S + off, M) if i >= M - N}
                for writer in fresh:
                    key = (c // n_loc, writer, form)
                    counts[key] = counts.get(key, 0) + 1
    return counts


def never_drawn(O, case, R):
    """Per member: the rows it appended that no later block-step of the run draws -- what only the archive comparison sees."""
    N, K, G = case["N"], case["K"], case["G"]
    n_loc, M0 = N // R, case["problem"]["Zinit"].shape[0]
    S, offs = _steps(case)
    drawn = np.zeros(M0 + N * (G // K), dtype=bool)
    for g in range(K + 1, G + 1):
        M = M0 + (g - 1) // K * N
        for c in range(N):
            for off in offs:
                i1, i2 = O.draw_rows(case["seed"], c, (g - 1) * S + off, M)
                drawn[i1] = drawn[i2] = True
    rank = (np.arange(M0, drawn.size) - M0) % N // n_loc
    return [int((~drawn[M0:] & (rank == r)).sum()) for r in range(R)]
