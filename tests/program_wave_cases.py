"""The worlds and schedules of the program-target tests on the wave-per-chain layout (no GPU, no assertions).

A handle created with lanes_per_chain = DEMCZ_LAYOUT_PROGRAM_WAVE runs the user's demcz_logobj in a hipRTC unit of its own
(demcz_program.hip, UNIT_WAVE): the general window_kernel_ps (d = 2..5) or window_kernel_pw (d = 6..32), each in four
instantiations LIVE x TEMPER, lane n = 1..31 of a chain's wave calling the program on candidate n of a five-generation pass.  Here:
for every d = 2..32 the MvNormal target restated as a program, the isotropic quadratic at five dimensions and Rosenbrock (no
built-in twin) at four, each with ONE schedule of demcz_run calls ("pieces") on one handle that reaches the four forms and passes
of every length inside and outside LIVE launches; and the named edges.  tests/test_program_wave_cases.py checks from the oracle
(or the oracle's loop around the Python twin) alone that these worlds are worth running; tests/test_gpu_program_wave_forms.py
compares the library with the same reference.

How a program handle cuts a call (demcz_capi.hip: demcz_run executes demcz_run_plan.h's plan_launch; a program handle on this
layout is a split handle of kind SPLIT_WAVE that is never a two-chain one -- demcz_create leaves ps_dual off for prog_wave -- and
window_kernel_of gives it ARM_PROGRAM_WAVE with the module [live][temper]: no regular / steady forms).  So the rules are those of
dimension_cases' docstring, K = 10 unless a world says otherwise:
  * a handle that can go LIVE (its consumer workgroups, four chains each, fit half the device together: every population here but
    PS_MAX_N) makes ONE launch of a call unless the launch before prepared fewer generations of draws than the call is long: it
    prepares as many as ITS call was long, nothing usable if that was shorter than K, and nothing before a first call or behind
    demcz_set_state.  A longer call behind a call of n >= K generations is cut at (n // K) * K; the rest is one launch;
  * LIVE: a K boundary lies inside the launch with a generation behind it -- (g_to - 1) // K > (g_from - 1) // K;
  * a handle that cannot go LIVE makes one launch per K-window, none of them LIVE;
  * tempered: the call has a temperature array.
"""
import numpy as np

import demc_jl_amd as demc
import dimension_cases as dc
import small_wave_cases as sw
from helpers import oracle_sample_logobj
from program_texts import ROSENBROCK, iso_program, mvn_program, rosenbrock_closure

PASS, K = dc.PASS, dc.K
DIMS = tuple(range(2, 33))
ISO_DIMS = (2, 5, 6, 19, 32)
ROSENBROCK_DIMS = (2, 5, 6, 32)
PS_MAX_N = 2048                   # demcz_kernels_ps.h
G_MAX = 500
# Chains of a main world with a built-in reference.  The siblings run d >= 6 with 96; here every tempered piece, the
# one-generation ones included, must depend on its temperatures in at least three chains (test_program_wave_cases.py); while the
# worlds were tuned against the oracle, 96 chains left such pieces with 0 .. 2 at the larger d.
N_MAIN = 192


def hot_of(kind, d):
    """The differences of log-density between a proposal and its chain grow with d in the MvNormal and isotropic worlds (the
    archive's starting rows stay far wider than the target), and a temperature changes a decision only where it is of their size."""
    return 3.0 if kind == "rosenbrock" else max(3.0, 0.625 * d)


def temperatures(G, hot=3.0):
    """Hot and cold generations in turn: dimension_cases.temperatures from `hot` down to half of it on the odd generations, the
    reciprocal of its fall from 3 to 1.5 on the even ones.  Its own fall from 3 to 0.5 passes through T = 1, where a short
    tempered piece is the untempered one for all but a chain or two and a kernel that ignored its temperatures would pass; and it
    changes by half a per cent from one generation to the next, where here a kernel that took a neighbouring generation's
    temperature divides by a number at least 2.25 times off."""
    T = dc.temperatures(G, hot=hot, cold=hot / 2.0)
    T[1::2] = 1.0 / dc.temperatures(G, hot=3.0, cold=1.5)[1::2]
    return T


LIVE_PLAIN, LIVE_TEMPERED, SHORT_PLAIN, SHORT_TEMPERED = FORMS = ("LIVE plain", "LIVE tempered", "non-LIVE plain", "non-LIVE tempered")

# the isotropic quadratic below d = 6 (dimension_cases has it from there on): about half of the proposals accepted
ISO_GAMMA = {2: 1.6, 5: 1.2}
# Rosenbrock, population 0.5 z + 0.5 (z standard normal), eps 1e-3: jumps at which a chain moves in 0.3 .. 0.7 of its generations,
# found on the CPU from the Python twin alone (test_program_wave_cases.py prints and holds the shares: 0.43 .. 0.58)
ROSENBROCK_GAMMA = {2: 0.5, 5: 0.25, 6: 0.22, 32: 0.06}
ROSENBROCK_N = 96


def form_of(g_from, g_to, tempered, k=K):
    """The form of a launch g_from..g_to."""
    return "%s %s" % ("LIVE" if (g_to - 1) // k > (g_from - 1) // k else "non-LIVE", "tempered" if tempered else "plain")


def kernel_name(d, form):
    live, tempered = form.split()
    return "demcz::window_kernel_%s<4, %d, %s, %s> (program)" % ("ps" if d <= 5 else "pw", d, "true" if live == "LIVE" else "false",
                                                                 "true" if tempered == "tempered" else "false")


def _pieces(lengths, k=K):
    pieces, g = [], 1
    for n, tempered in lengths:
        pieces.append((g, g + n - 1, tempered, form_of(g, g + n - 1, tempered, k)))
        g += n
    return pieces


def crossing(s, e, tempered):
    """Two K-windows: a LIVE piece that starts s generations before the boundary between them and ends e behind it (passes of s and
    e generations inside a LIVE launch), in front of it the first window's other 10 - s generations (passes of 5 and 5 - s), behind
    it the second window's other 10 - e (5 and 5 - e), the one with the piece's temperatures, the other without."""
    return [(K - s, tempered), (s + e, tempered), (K - e, not tempered)]


def schedule():
    """[(g_from, g_to, tempered, form)], tiling 1..480.  The first eleven pieces of dimension_cases.pw_schedule (which
    small_wave_cases.one_schedule starts with as well; the second one plain here): LIVE launches of 40 and 43 generations, plain and tempered, each behind a
    short piece, five-generation pieces around them.  Then crossings (s, e) = (1, 4), (2, 3), (3, 2), (4, 1), plain and tempered,
    and (4, 4), (3, 4), (4, 3) again: every pass length 1..4 inside LIVE launches of either kind, and in the non-LIVE pieces
    around them.  Then small_wave_cases.WINDOW_PAIR (windows cut 2 + 5 + 3 and 1 + 5 + 4) plain, then tempered."""
    lengths = [(b - a + 1, t) for a, b, t, _ in dc.pw_schedule()[:11]]             # ..200
    lengths[1] = (5, False)         # (6..10: the population is still far from the target, and no temperature changes a decision)
    for s, e in ((1, 4), (2, 3), (3, 2), (4, 1)):                                    # ..360
        lengths += crossing(s, e, False) + crossing(s, e, True)
    for s, e in ((4, 4), (3, 4)):                                                    # ..440
        lengths += crossing(s, e, True) + crossing(s, e, False)
    for i in range(2):                                                               # ..480
        lengths += [(n, i % 2 == 1) for n in sw.WINDOW_PAIR]
    return _pieces(lengths)


def launch_pieces(case):
    """The case's pieces as launches, by the rules of this module's docstring: [(g_from, g_to, tempered, form)] with a cut call in
    its two launches and, on a handle that cannot go LIVE, every piece in its K-windows."""
    k, out, prepared = case["K"], [], 0
    for a, b, tempered, _ in case["pieces"]:
        n = b - a + 1
        if not case["live"]:
            ends = [min(e, b) for e in range(((a - 1) // k + 1) * k, b + k, k)]
        elif prepared >= k and n > prepared:
            ends = [a + (prepared // k) * k - 1, b]          # (the first launch prepares the rest)
        else:
            ends = [b]
        g = a
        for e in ends:
            out.append((g, e, tempered, form_of(g, e, tempered, k) if case["live"] else "non-LIVE " + ("tempered" if tempered else "plain")))
            g = e + 1
        prepared = 0 if b == case["resume_at"] else n        # (demcz_set_state discards what was prepared)
    return out


def launches_after(case):
    """The count of window launches behind every piece."""
    ends = [l[1] for l in launch_pieces(case)]
    return [sum(1 for e in ends if e <= b) for _, b, _, _ in case["pieces"]]


def _world(name, kind, d, N, gamma, problem, program, pieces, seed, k=K, temperature=None, **more):
    G = pieces[-1][1]
    case = dict(name=name, kind=kind, d=d, N=N, K=k, seed=seed, gamma=gamma, problem=problem, program=program, pieces=pieces, G=G,
                temperature=temperatures(G, hot_of(kind, d)) if temperature is None else temperature, live=True, history=True, resume_at=None)
    case.update(more)
    return case


def _mvn_problem(d, N):
    w = demc.workloads.mvnormal_problem(d, N)
    return w, lambda: mvn_program(w["target"].mu, w["target"].W, w["target"].c0)


def _iso_problem(d, N):
    w = demc.workloads.iso_quad_problem(d, N)
    return w, lambda: iso_program(w["mu"])


def _sibling(kind, d):
    """Chains, and the jump and seed of the sibling world of the built-in kernels."""
    if d <= 5:
        c = sw.small_case(d, False)
        gamma = c["gamma"] if kind == "mvn" else ISO_GAMMA[d]
    else:
        c = dc.pw_case(kind, d)
        # (MvNormal at d = 6..10: 0.2 moves a chain in two generations of three and more, and a pass of three in which it never
        #  moves is not seen inside a tempered LIVE launch; the jumps of the replicated consumer's worlds there)
        gamma = sw.PC8_GAMMA[kind, d] if (kind, d) in sw.PC8_GAMMA else c["gamma"]
    return N_MAIN, gamma, c["seed"] + (kind == "iso" and d <= 5)


def mvn_case(d):
    """MvNormal restated as a program at d in 2..32; the reference is the oracle's built-in MvNormal."""
    N, gamma, seed = _sibling("mvn", d)
    w, prog = _mvn_problem(d, N)
    return _world("mvn_d%d" % d, "mvn", d, N, gamma, w, prog, schedule(), seed)


def iso_case(d):
    N, gamma, seed = _sibling("iso", d)
    w, prog = _iso_problem(d, N)
    return _world("iso_d%d" % d, "iso", d, N, gamma, w, prog, schedule(), seed)


def rosenbrock_case(d):
    """A program with no built-in twin, data = NULL, ndata = 0; the reference is helpers.oracle_sample_logobj around
    program_texts.rosenbrock_closure (twin_run below)."""
    N = ROSENBROCK_N
    r = np.random.default_rng(20261019 + d)
    Zinit = np.asfortranarray(0.5 * r.standard_normal((max(10 * d, N) + N, d)) + 0.5)
    problem = dict(Zinit=Zinit, eps_scale=1e-3 * np.ones(d), target=None)
    return _world("rosenbrock_d%d" % d, "rosenbrock", d, N, ROSENBROCK_GAMMA[d], problem, lambda: demc.ProgramTarget(ROSENBROCK, d),
                  schedule(), 20261019 + 17 * d, logobj=rosenbrock_closure)


MAIN_WORLDS = tuple(("mvn", d) for d in DIMS) + tuple(("iso", d) for d in ISO_DIMS) + tuple(("rosenbrock", d) for d in ROSENBROCK_DIMS)


def main_case(kind, d):
    return {"mvn": mvn_case, "iso": iso_case, "rosenbrock": rosenbrock_case}[kind](d)


# ---- named edges: each one small world (MvNormal as a program, the world's own gamma) -----------------------------------------------
def edge_case(tag, d, N, lengths, k=K, temperature=None, **more):
    _, gamma, _ = _sibling("mvn", d)
    w, prog = _mvn_problem(d, N)
    return _world("%s_d%d_N%d_K%d" % (tag, d, N, k), "mvn", d, N, gamma, w, prog, _pieces(lengths, k), 20261019 + 31 * d + 7 * N + k, k=k,
                  temperature=temperature, **more)


TINY = tuple((d, N) for d in (3, 7) for N in (1, 3, 5, 9))          # idle chain waves in a four-chain workgroup, a ragged last one


def tiny_case(d, N):
    return edge_case("tiny", d, N, sw.TINY_LENGTHS)                 # non-LIVE plain, LIVE tempered, non-LIVE tempered, LIVE plain


def largest_case():
    """N = PS_MAX_N at d = 5: 512 consumer workgroups do not fit half the device together -- never LIVE, one launch per K-window."""
    return edge_case("largest", 5, PS_MAX_N, [(13, False), (12, True)], live=False)


# K -> the lengths of a plain and a tempered call, each from a window's start and as long as the call before or shorter (one
# launch each, K = 1 included, where no piece is shorter than K); the pass lengths these produce
OTHER_K = {1: ([(30, False), (30, True)], (1,)), 3: ([(30, False), (30, True)], (3,)), 4: ([(32, False), (32, True)], (4,)),
           7: ([(35, False), (28, True)], (5, 2)), 12: ([(36, False), (24, True)], (5, 2))}
OTHER_K_DIMS = (4, 9)


def other_k_case(d, k):
    return edge_case("other_K", d, 96, OTHER_K[k][0], k=k)


CUT_DIMS = (3, 8)


def cut_case(d):
    """small_wave_cases.CUT_LENGTHS / CUT_K: a tempered call of 45 generations behind a call of 15, K = 5, is cut behind its
    fifteenth generation; its second launch reads its temperatures from an odd offset into the call's array."""
    return edge_case("cut", d, 37, sw.CUT_LENGTHS, k=sw.CUT_K)


EDGE_TEMPERATURE_DIMS = (2, 5, 6, 32)


def edge_temperature_case(d):
    return edge_case("edge_T", d, 37, [(60, True)], temperature=sw.temps_with_zeros(60))


NO_HISTORY_DIMS = (4, 7)


def no_history_case(d):
    """Gcap = 0: every history store of a pass is out of the (empty) buffer's range by design."""
    return edge_case("no_history", d, 37, [(40, True)], history=False)


RESUME_AT = 12                    # inside a window
RESUMED_DIMS = (3, 8)


def resumed_case(d):
    """Behind generation RESUME_AT the handle is given its own state back (demcz_set_state): nothing is prepared for the piece that
    follows, and changed_total is asked from generation RESUME_AT + 1 on (the state's log-densities become what the history's
    first generation is counted against)."""
    return edge_case("resumed", d, 190, [(3, False), (RESUME_AT - 3, False), (3, False), (12, False), (2, True), (11, True)], resume_at=RESUME_AT)


def edge_worlds():
    """{name: case maker} of every edge world the GPU file runs."""
    makers = {}
    for d, N in TINY:
        makers["tiny_d%d_N%d" % (d, N)] = lambda d=d, N=N: tiny_case(d, N)
    makers["largest"] = largest_case
    for d in OTHER_K_DIMS:
        for k in OTHER_K:
            makers["K%d_d%d" % (k, d)] = lambda d=d, k=k: other_k_case(d, k)
    for d in CUT_DIMS:
        makers["cut_d%d" % d] = lambda d=d: cut_case(d)
    for d in EDGE_TEMPERATURE_DIMS:
        makers["edge_T_d%d" % d] = lambda d=d: edge_temperature_case(d)
    for d in NO_HISTORY_DIMS:
        makers["no_history_d%d" % d] = lambda d=d: no_history_case(d)
    for d in RESUMED_DIMS:
        makers["resumed_d%d" % d] = lambda d=d: resumed_case(d)
    return makers


def kernel_names_planned():
    """Every kernel name the main worlds assert."""
    return {kernel_name(d, p[3]) for d in DIMS for p in schedule()}


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def twin_run(O, case, pieces=None, start=None, tempered=True):
    """The oracle's loop around the case's Python twin over the pieces (default: the case's), from `start` = (X, lp, Z) (default:
    the case's starting state).  dimension_cases.oracle_run's dict."""
    w, N, d, k = case["problem"], case["N"], case["d"], case["K"]
    pieces = case["pieces"] if pieces is None else pieces
    g0, G = pieces[0][0], pieces[-1][1] - pieces[0][0] + 1
    if start is None:
        Z = np.array(w["Zinit"], order="F")
        X, lp = np.array(Z[-N:], order="F"), None
    else:
        X, lp, Z = (np.array(v, order="F") for v in start)
    chain, lobj, changed, lp0 = np.zeros((N, d, G), order="F"), np.zeros((N, G), order="F"), np.zeros(G, dtype=np.int64), None
    for p in pieces:
        a, b = p[0], p[1]
        T = case["temperature"][a - 1:b] if (p[2] and tempered) else None
        r = oracle_sample_logobj(O, case["logobj"], Z, N, k, b - a + 1, None, w["eps_scale"], case["gamma"], case["seed"], temperature=T,
                                 X0=X, lp0=lp, g_from=a)
        if lp0 is None:
            lp0 = np.array([case["logobj"]([float(v) for v in x]) for x in X]) if lp is None else np.array(lp)
        chain[:, :, a - g0:b - g0 + 1], lobj[:, a - g0:b - g0 + 1], changed[a - g0:b - g0 + 1] = r["chain"], r["log_obj"], r["changed"]
        X, lp, Z = r["X"], r["logp"], r["Z"]
    return dict(chain=chain, log_obj=lobj, X=X, logp=lp, Z=Z, M=Z.shape[0], changed=changed, lp0=lp0)


_RUNS = {}


def reference_run(O, case):
    """The reference of a world, computed once per process and left unchanged: the oracle's built-in target, or the oracle's loop
    around the Python twin."""
    if case["name"] not in _RUNS:
        r = twin_run(O, case) if "logobj" in case else dc.oracle_run(O, case)
        r["X0"] = np.array(case["problem"]["Zinit"][-case["N"]:], order="F")
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[case["name"]] = r
    return _RUNS[case["name"]]


def untempered_differences(O, case, ref):
    """Per tempered piece: the number of chains whose history inside the piece differs when the reference is started again at the
    piece's start from its own state there and runs the piece WITHOUT its temperatures."""
    N, k, d, out = case["N"], case["K"], case["d"], []
    M0 = case["problem"]["Zinit"].shape[0]
    for a, b, tempered, _ in case["pieces"]:
        if not tempered:
            continue
        X = np.array(ref["chain"][:, :, a - 2] if a > 1 else ref["X0"], order="F")
        lp = np.array(ref["log_obj"][:, a - 2] if a > 1 else ref["lp0"])
        M = M0 + N * ((a - 1) // k)
        if "logobj" in case:
            r = twin_run(O, case, pieces=[(a, b, True, "")], start=(X, lp, ref["Z"][:M]), tempered=False)
        else:
            w = case["problem"]
            Z = np.zeros((M + N * ((b - a) // k + 2), d), order="F")
            Z[:M] = ref["Z"][:M]
            prob = O.Problem(N, d, k, Z.shape[0], w["eps_scale"], case["seed"], target=w["target"].spec())
            _, ch, _, _ = O.run(prob, X, lp, Z, M, a, b, case["gamma"], temperature=None)
            r = dict(chain=ch)
        out.append(int((r["chain"] != ref["chain"][:, :, a - 1:b]).any(axis=(1, 2)).sum()))
    return out


def short_pass_outcomes(case, log_obj, lp0, length):
    """{form: counts[2 ** length]} over the passes of `length` generations of the case's pieces (cut into their launches where a
    piece is more than one: a launch's end ends a pass)."""
    return dc.pass_outcomes(launch_pieces(case), log_obj, lp0, k=case["K"], forms=FORMS, length=length)
