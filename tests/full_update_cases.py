"""The worlds and schedules of the full-update tests (no GPU, no assertions).

One block 0..d-1 in order runs on kernels of its own (demcz_capi.hip: window_kernel_of).  The wave-per-chain ones (ps / ps2 / ps2d /
pw), the replicated consumer pc8 and the sixteen-lane regression kernel at every d have every-form tests; here are the others:
  A. window_kernel_ml, lanes of a wave sharing a chain: fused <MVNORMAL, 2..10, 8>, <ISO_QUAD, 10, 8>, <MVNORMAL, 20, 16>, a launch
     per K-window, plain and tempered at run time; split <MVNORMAL, 20, 16, true, LIVE> -- 13 instantiations;
  B. the d = 10 regression target on the FP64 matrix instruction (demcz_kernels_lr.h): window_kernel_lr16<10, false, false> fused,
     window_kernel_lr16<10, true, LIVE> and window_kernel_lr8s<10, LIVE> split -- design and observations live in LDS, so the
     observation count decides which of them fit;
  C. window_kernel<TARGET, D, true>, one lane per chain: MvNormal 2, 3, 4, 5, 8, 10, 20, iso-quad 10, regression 10 and 26, and
     window_kernel_generic<TARGET> at any other dimension.
As in tests/block_cases.py (whose schedule, temperatures, oracle runs and counts these worlds use): per world ONE handle per layout
whose schedule of demcz_run calls ("pieces") reaches every form, the oracle's run of it -- which does not depend on the layout, so
a world (kind, d, gamma) serves every layout built for it -- and the planned kernel names and launch counts.
tests/test_full_update_cases.py checks the worlds from the oracle alone, tests/test_gpu_full_update_forms.py compares the library.

Which form a piece runs (demcz_run_plan.h; K = 5): see block_cases' docstring.  The fused and the one-lane layouts launch once per
K-window; a split handle that goes LIVE runs a piece as one launch while the draws prepared for it reach (split_live_launches).
"""
import demc_jl_amd as demc

import block_cases as bc
import dimension_cases as dc
from block_cases import EDGE_LENGTHS, FORMS, K, LR_NOBS, MI355X_CUS, N_MAIN, RESUME_AT, TARGET_NAME, pieces_of, schedule

NO_LR_SPEC = "DEMCZ_NO_LR_SPEC"               # read in demcz_create: the split regression handle stays on sixteen chains a workgroup

# ---- worlds -------------------------------------------------------------------------------------------------------------------------
# id -> (kind, d, N, gamma).  The workload's 2.38 moves a chain in a few per cent of its generations; at these jumps it moves in
# about half of them.  Measured with the oracle on the full schedule (tests/test_full_update_cases.py prints them): the share of
# (chain, generation) that moved | the rarest (previous outcome, this outcome) pair over the four forms | the fewest chains a
# tempered piece changes when it is run without its temperatures.
WORLDS = {
    "mvn2": ("mvn", 2, N_MAIN, 0.9),                # 0.391 | 155 | 40
    "mvn3": ("mvn", 3, N_MAIN, 0.7),                # 0.383 | 224 | 31
    "mvn4": ("mvn", 4, N_MAIN, 0.55),               # 0.412 | 275 | 34
    "mvn5": ("mvn", 5, N_MAIN, 0.45),               # 0.438 | 312 | 29
    "mvn6": ("mvn", 6, N_MAIN, 0.4),                # 0.450 | 355 | 18
    "mvn7": ("mvn", 7, N_MAIN, 0.35),               # 0.435 | 309 | 11
    "mvn8": ("mvn", 8, N_MAIN, 0.3),                # 0.464 | 369 | 11
    "mvn9": ("mvn", 9, N_MAIN, 0.28),               # 0.483 | 432 |  9
    "mvn10": ("mvn", 10, N_MAIN, 0.25),             # 0.468 | 367 | 10
    "mvn20": ("mvn", 20, N_MAIN, 0.25),             # 0.464 | 439 |  5
    "iso10": ("iso", 10, N_MAIN, 1.2),              # 0.526 | 232 | 48
    "mvn13": ("mvn", 13, N_MAIN, 0.22),             # 0.491 | 448 | 10
    "mvn64": ("mvn", 64, N_MAIN, 0.08),             # 0.605 |  27 | 41
    "iso7": ("iso", 7, N_MAIN, 1.2),                # 0.531 | 182 | 36
    "lr10": ("lr", 10, N_MAIN, 0.5),                # 0.567 | 132 | 45
    "lr26": ("lr", 26, N_MAIN, 0.3),                # 0.576 | 226 | 26
    "lr7": ("lr", 7, N_MAIN, 0.5),                  # 0.568 |  90 | 34
    # B: two and a half workgroups of window_kernel_lr16 (sixteen chains each), five of window_kernel_lr8s (eight)
    "lr10_matrix": ("lr", 10, 40, 0.5),             # 0.573 |  33 | 14
}
FUSED_LANES = {("mvn", d): 8 for d in range(2, 11)}
FUSED_LANES.update({("mvn", 20): 16, ("iso", 10): 8, ("lr", 10): 16})
FUSED_WORLDS = tuple("mvn%d" % d for d in range(2, 11)) + ("mvn20", "iso10")
SPLIT_WORLDS = ("mvn20",)
ONE_LANE_WORLDS = ("mvn2", "mvn3", "mvn4", "mvn5", "mvn8", "mvn10", "mvn20", "mvn7", "mvn13", "mvn64", "iso10", "iso7", "lr10", "lr26", "lr7")
LR_WORLD = "lr10_matrix"
# the three handles of B: (layout, environment switches)
LR_HANDLES = (("fused", ()), ("split", ()), ("split", (NO_LR_SPEC,)))
LR_HANDLE_IDS = ("lr16", "lr8s", "lr16_split")


def case_of(name, N=None, pieces=None, nobs=None, temperature=None, tag=None):
    """A world of the table, on the full schedule under its own name, or at another population / observation count / schedule under
    a name that says so (the oracle's runs are kept by name)."""
    kind, d, n, gamma = WORLDS[name]
    N = n if N is None else N
    nobs = (LR_NOBS if nobs is None else nobs) if kind == "lr" else None
    # ("full_": block_cases keeps the oracle's runs by name, and its own one-lane block worlds are called iso10, lr10, ... too)
    cname = "full_" + (name if tag is None else "%s_%s_N%d%s" % (tag, name, N, "_nobs%d" % nobs if kind == "lr" else ""))
    problem = demc.workloads.linreg_problem(d, N, nobs=nobs) if kind == "lr" else None
    case = bc._case(cname, kind, d, [list(range(d))], N, gamma, schedule() if pieces is None else pieces, (), temperature, problem=problem)
    case["nobs"] = nobs
    return case


# ---- the LDS of the matrix kernels (demcz_kernels_lr.h, restated) ---------------------------------------------------------------------
LDS_LIMIT = 160 * 1024                    # ML_MAX_DYNAMIC_LDS (demcz_capi.hip): the LDS of a CU
LR16_WAVES, LR16_CHAINS, LR8_CHAINS, LR8_RING, LR8_IXRING = 4, 16, 8, 4, 8


def lr16_lds(nobs, d=10):
    """lr16_dynamic_lds<D>: the design in A-operand order (per group of 64 observations, wave and k-step of four columns: 64
    doubles), the observations (per group and wave: 16), the partials of two generations (rows of 18 doubles), the draws of a
    generation (S blocks of 16 bytes a chain), two flag words."""
    nmf, s = (d + 3) // 4, (1 if d == 1 else (d + 1) // 2) + 2
    ngrp = (nobs + 63) // 64
    return ngrp * LR16_WAVES * nmf * 64 * 8 + ngrp * LR16_WAVES * 16 * 8 + 2 * LR16_CHAINS * 18 * 8 + LR16_CHAINS * s * 16 + 16


def lr8s_lds(nobs, d=10):
    """lr8s_dynamic_lds<D>: lr16's, and per wave a ring of four generations per chain (32 doubles each, + 4), the row indices' ring
    and a generation counter per chain."""
    ch_doubles = LR8_RING * 32 + 4
    return lr16_lds(nobs, d) + LR16_WAVES * (LR8_CHAINS * ch_doubles * 8 + LR8_CHAINS * LR8_IXRING * 8 + LR8_CHAINS * 4)


def max_obs(lds):
    """The largest observation count whose LDS (a function of ceil(nobs / 64)) fits a CU."""
    n = 64
    while lds(n + 64) <= LDS_LIMIT:
        n += 64
    return n


LR8S_MAX_OBS, LR16_MAX_OBS = max_obs(lr8s_lds), max_obs(lr16_lds)
NOBS_COUNTS = (1, 3, 4, 15, 16, 17, 63, 64, 65, 128)         # a tile of 16, a group of 64 and their neighbours
LR_POPULATIONS = (1, 7, 9, 15, 17, 33)                        # idle columns shadow chain N - 1, at 16 and 8 chains per workgroup
# (nobs, layout, environment) at the limits of the fit rules; LR16_MAX_OBS + 1 on the split layout is refused by demcz_create
LR_LIMITS = ((LR8S_MAX_OBS, "split", ()), (LR8S_MAX_OBS + 1, "split", ()), (LR16_MAX_OBS, "fused", ()), (LR16_MAX_OBS, "split", ()),
             (LR16_MAX_OBS + 1, "fused", ()))


def lr_case(nobs=LR_NOBS, N=None):
    """B's world at another observation count or population: 25 generations, every form."""
    return case_of(LR_WORLD, N=N, nobs=nobs, pieces=pieces_of(EDGE_LENGTHS), tag="edge")


# ---- kernel names ---------------------------------------------------------------------------------------------------------------------
def planned_name(case, layout, form, env=()):
    """What demcz_debug_kernel_name must say behind a piece of `form`; layout: "fused", "split", "one"."""
    kind, d = case["kind"], case["d"]
    live = "true" if form.startswith("LIVE") else "false"
    if layout == "one":
        # (a dimension without a specialisation launches window_kernel_generic<TARGET> and is reported under this name all the
        #  same: demcz_debug_kernel_name's known misreport)
        return "demcz::window_kernel<%s, %d, true>" % (TARGET_NAME[kind], d)
    if kind == "lr":
        nobs = case["nobs"]
        if layout == "fused":
            return dc.lr_kernel_name(d, nobs <= dc.ML_COOP_MAX_OBS, lr16_fits=lr16_lds(nobs) <= LDS_LIMIT)
        if NO_LR_SPEC not in env and lr8s_lds(nobs) <= LDS_LIMIT and -(-case["N"] // LR8_CHAINS) <= MI355X_CUS:
            return "demcz::window_kernel_lr8s<%d, %s>" % (d, live)
        return "demcz::window_kernel_lr16<%d, true, %s>" % (d, live)
    if layout == "fused":
        return "demcz::window_kernel_ml<%s, %d, %d>" % (TARGET_NAME[kind], d, FUSED_LANES[kind, d])
    return "demcz::window_kernel_ml<%s, %d, 16, true, %s>" % (TARGET_NAME[kind], d, live)


def one_lane_specialised(kind, d):
    return d in {"mvn": (2, 3, 4, 5, 8, 10, 20), "iso": (10,), "lr": (10, 26)}[kind]


# ---- launch counts (demcz_run_plan.h, plan_launch) -------------------------------------------------------------------------------------
def split_live_launches(pieces, k=K, cold_behind=()):
    """The count of window launches behind every piece of a split handle that goes LIVE, with a span longer than any piece and no
    hint of the next call.  A launch's producer half prepares the draws of the launch behind it: the rest of its call, or as many
    generations as its call was long.  A launch runs to its call's end when no draws of at least K generations are there for it
    (they are made first: a cold start) or when they reach; otherwise it is cut to the whole K-windows prepared.  cold_behind:
    generations behind which demcz_set_state has thrown the prepared draws away."""
    out, n, prepared = [], 0, 0
    for a, b, _, _ in pieces:
        g = a
        while g <= b:
            m = b - g + 1
            if k <= prepared < m:
                m = max(prepared // k * k, k)
            g += m
            n += 1
            prepared = b - g + 1 if g <= b else b - a + 1
        if b in cold_behind:
            prepared = 0
        out.append(n)
    return out


def plan(case, layout, env=(), live=True, cold_behind=()):
    """[(kernel name, window launches behind the piece)] of a handle.  live = False: a split handle that the device does not hold
    in one LIVE launch runs every piece in the non-LIVE form, one launch per K-window."""
    pieces = case["pieces"]
    if layout == "split" and live:
        counts = split_live_launches(pieces, case["K"], cold_behind)
        return [(planned_name(case, layout, p[3], env), c) for p, c in zip(pieces, counts)]
    return [(planned_name(case, layout, "non-LIVE", env), c) for c in bc.per_window_launches(pieces, case["K"])]


def last_launch_from(case, layout, live=True):
    """The first generation of the handle's last window launch: changed_total from there is one launch's ballots."""
    a, b = case["pieces"][-1][:2]
    return a if layout == "split" and live else max(a, (b - 1) // case["K"] * case["K"] + 1)


# ---- four-wave workgroups ---------------------------------------------------------------------------------------------------------------
# The library takes workgroups of four chain waves when ceil(N L / 64) >= 4 CUs (demcz_create: wpw; the kernel: gq = wv NG + lane / L,
# vb = block wpw + wv).  N = 4 CUs (64 / L) + 5 (L = 8) or + 3 (L = 16): one workgroup more than CUs, only partly filled.  The split
# d = 20 handle also at - 3; whether such a handle goes LIVE is the device's matter (live_wg_capacity) and its LIVE status decides
# the plan it is held to.  d = 9 and 10: a lane owns two parameters.  A piece inside a window, one across two boundaries, a window.
FOUR_WAVE_FUSED = ("mvn2", "mvn5", "mvn9", "mvn10", "iso10", "mvn20")
FOUR_WAVE_SPLIT = (("mvn20", 1), ("mvn20", -1))
FOUR_WAVE_LENGTHS = [(3, True), (2 * K, False), (K, True)]


def lanes_of(case):
    return FUSED_LANES[case["kind"], case["d"]]


def four_wave_case(name, sign=1, cus=MI355X_CUS):
    kind, d = WORLDS[name][:2]
    L = FUSED_LANES[kind, d]
    N = 4 * cus * (64 // L) + (5 if L == 8 else 3) * sign
    return case_of(name, N=N, pieces=pieces_of(FOUR_WAVE_LENGTHS), tag="four_wave")


def chain_waves(case):
    return (case["N"] * lanes_of(case) + 63) // 64


# ---- named edges ------------------------------------------------------------------------------------------------------------------------
TINY = [(w, N, "fused") for w in ("mvn3", "mvn9") for N in (1, 3, 5, 9)] + [("mvn20", N, lay) for N in (1, 3, 5) for lay in ("fused", "split")]
NO_HISTORY = (("mvn7", "fused"), ("mvn20", "split"))
ZERO_TEMPERATURE = (("mvn4", "fused"), ("mvn20", "fused"), ("mvn20", "split"))
RESUMED = (("mvn6", "fused"), ("mvn20", "split"))
ONE_LANE_POPULATIONS = [(w, N) for w in ("mvn5", "mvn7") for N in (1, 63, 64, 65, 129)]       # WINDOW_BS = 64 chains a workgroup
ZERO_LENGTHS = [(3, True), (27, True), (5, True), (2, True), (3, True)]
RESUMED_LENGTHS = [(3, False), (RESUME_AT - 3, False), (3, False), (12, False), (2, True), (11, True)]


def edge_case(name, N=None):
    return case_of(name, N=N, pieces=pieces_of(EDGE_LENGTHS), tag="edge")


def zero_temperature_case(name):
    from small_wave_cases import temps_with_zeros
    return case_of(name, pieces=pieces_of(ZERO_LENGTHS), temperature=temps_with_zeros(40), tag="zero_temperature")


def resumed_case(name):
    """Two parts of one run: the handle is given its own state back behind generation RESUME_AT, in the middle of a window."""
    return case_of(name, pieces=pieces_of(RESUMED_LENGTHS), tag="resumed")


# ---- everything the GPU tier runs ----------------------------------------------------------------------------------------------------------
def main_runs():
    """[(case, layout, environment)] of the full schedule: every main world on every handle it has."""
    runs = [(case_of(w), "fused", ()) for w in FUSED_WORLDS] + [(case_of(w), "split", ()) for w in SPLIT_WORLDS]
    runs += [(case_of(LR_WORLD), lay, env) for lay, env in LR_HANDLES]
    return runs + [(case_of(w), "one", ()) for w in ONE_LANE_WORLDS]


def edge_runs(cus=MI355X_CUS):
    """[(case, layout, environment)] of the four-wave worlds and the named edges."""
    runs = [(four_wave_case(w, 1, cus), "fused", ()) for w in FOUR_WAVE_FUSED] + [(four_wave_case(w, s, cus), "split", ()) for w, s in FOUR_WAVE_SPLIT]
    runs += [(edge_case(w, N), lay, ()) for w, N, lay in TINY] + [(edge_case(w), lay, ()) for w, lay in NO_HISTORY]
    runs += [(zero_temperature_case(w), lay, ()) for w, lay in ZERO_TEMPERATURE] + [(resumed_case(w), lay, ()) for w, lay in RESUMED]
    runs += [(lr_case(nobs), lay, env) for nobs in NOBS_COUNTS for lay, env in LR_HANDLES]
    runs += [(lr_case(nobs), lay, env) for nobs, lay, env in LR_LIMITS]
    runs += [(lr_case(N=N), lay, env) for N in LR_POPULATIONS for lay, env in LR_HANDLES]
    return runs + [(edge_case(w, N), "one", ()) for w, N in ONE_LANE_POPULATIONS]


def kernel_names_planned():
    return {name for case, lay, env in main_runs() + edge_runs() for name, _ in plan(case, lay, env)}
