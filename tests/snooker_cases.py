"""The worlds tests/test_gpu_snooker.py and tests/test_gpu_snooker_forms.py run against tests/snooker_reference.py, and what the
reference alone must show of each (tests/test_snooker_cases.py) for the bit comparison to be worth making.

A main world: N = 70 chains (one full wave and a part-filled one), G = 40 generations, an archive of N + 40 rows whose last N are
the chains' starting states (so 40 rows are archive-only), K in {3, 10}, snooker generations every 1, 3 or K generations.  The
populations start overdispersed about their targets, not at standard normals: a snooker step is accepted or rejected by its
log-density difference and its Jacobian together, and far out in a tail almost every step goes one way.

WORLDS are the 16 of the snooker update's first tests (tests/test_gpu_snooker.py runs exactly these); NEW_WORLDS reach what they
left out -- the five specialised instantiations never launched (MvNormal 3, 4, 8, 10; regression 26), the grouped branch of the
specialised kernel (scalar-register and memory form), MAX_D = 64, tempered steps in every kernel family, MvNormal restated as a
program at the ends of the program range against the ORACLE'S built-in log-density, a straight-line program at d = 32; MAIN is
both.  EDGE_WORLDS are small worlds at the edges of the launch: populations of 1 and 2, archives of exactly three rows, populations
about the 64-chain workgroup, K = 1, snooker generations rarer than the run is long or one off the K-window, own-row anchors and
+-inf rows in the specialisations with scalar-register whitening, gamma_lo == gamma_hi.

What tests/test_snooker_cases.py asks of every MAIN world (each threshold 3 unless stated):
  * at least 10 accepted and 10 rejected snooker steps, both outcomes in the part-filled wave;
  * the Jacobian's exponent matters: valid steps whose decision differs with (d - 2) / 2 and with d / 2 in place of (d - 1) / 2;
  * both outcomes among the snooker generations that are multiples of K, and among those that are not where the world has such;
  * the worlds marked needs_invalid show steps whose |x - a|^2 or |x' - a|^2 is no positive normal double;
  * tempered worlds: steps whose decision differs with T ignored, steps whose decision differs with the Jacobian tempered too, and
    T = 0, 1e-300 and 1e300 each at a snooker generation.  The new tempered worlds have one plain piece (no temperatures) as well;
  * grouped worlds: ACCEPTED steps whose proposal has other log-density bits in the ungrouped summation order; the interleaved
    structure of mvn8_inter shows none (it is not a grouping).
Of every EDGE world with N >= 63: both outcomes in its last wave; of the three-row worlds one accepted, one rejected, three invalid.

Measured with the oracle (accepted / valid rejected / invalid of all snooker steps; flips at exponent d - 2, d; accepted / rejected
at multiples of K; accepted / rejected elsewhere):
  mvn2                    317 / 592 / 1      77, 55    317 / 592    0 / 0
  mvn5                    63 / 217 / 0       12, 12    63 / 217     0 / 0
  mvn5_all                800 / 1993 / 7     109, 106  240 / 670    560 / 1323
  mvn7                    221 / 688 / 1      19, 20    11 / 59      210 / 629
  mvn20                   196 / 713 / 1      7, 10     196 / 713    0 / 0
  mvn33                   401 / 2394 / 5     12, 8     30 / 250     371 / 2144
  iso10                   301 / 604 / 5      27, 26    22 / 48      279 / 556
  iso6                    961 / 1835 / 4     130, 121  284 / 626    677 / 1209
  lr10                    297 / 613 / 0      14, 20    297 / 613    0 / 0
  lr4                     85 / 195 / 0       14, 13    85 / 195     0 / 0
  rosenbrock7             227 / 681 / 2      6, 5      18 / 52      209 / 629
  box4                    300 / 608 / 2      61, 49    300 / 608    0 / 0
  mvn6_blocks             222 / 688 / 0      27, 31    21 / 49      201 / 639    grouped differ 337, accepted 68
  mvn5_tempered           413 / 495 / 2      30, 10    22 / 48      391 / 447    decisions with T ignored 252 with the Jacobian tempered 151
  mvn5_own_row            768 / 2026 / 6     109, 94   86 / 194     682 / 1832
  iso6_inf                310 / 577 / 23     31, 34    310 / 577    0 / 0
  mvn3                    275 / 633 / 2      48, 46    275 / 633    0 / 0
  mvn4                    259 / 650 / 1      37, 31    21 / 49      238 / 601
  mvn8                    230 / 680 / 0      26, 14    230 / 680    0 / 0
  mvn10                   194 / 712 / 4      19, 13    10 / 60      184 / 652
  lr26                    330 / 575 / 5      11, 6     330 / 575    0 / 0
  lr7                     291 / 616 / 3      31, 34    291 / 616    0 / 0
  mvn64_all               353 / 2436 / 11    8, 5      23 / 257     330 / 2179
  iso64                   344 / 564 / 2      9, 5      344 / 564    0 / 0
  mvn10_halves            200 / 709 / 1      12, 10    12 / 58      188 / 651    grouped differ 352, accepted 67
  mvn20_4x5               200 / 706 / 4      10, 12    200 / 706    0 / 0        grouped differ 479, accepted 87
  mvn8_inter              223 / 683 / 4      20, 17    223 / 683    0 / 0        grouped differ 0, accepted 0
  mvn8_tempered           328 / 579 / 3      13, 9     31 / 39      297 / 540    decisions with T ignored 197 with the Jacobian tempered 131
  mvn20_tempered          343 / 567 / 0      3, 5      28 / 42      315 / 525    decisions with T ignored 209 with the Jacobian tempered 170
  mvn13_tempered          344 / 563 / 3      3, 5      26 / 44      318 / 519    decisions with T ignored 196 with the Jacobian tempered 154
  mvn10_halves_tempered   326 / 583 / 1      11, 6     33 / 37      293 / 546    grouped differ 405, accepted 146 decisions with T ignored 193 with the Jacobian tempered 150
  iso10_tempered          433 / 475 / 2      14, 13    433 / 475    0 / 0        decisions with T ignored 226 with the Jacobian tempered 164
  iso6_tempered           403 / 507 / 0      27, 23    403 / 507    0 / 0        decisions with T ignored 210 with the Jacobian tempered 146
  lr10_tempered           402 / 507 / 1      14, 8     32 / 38      370 / 469    decisions with T ignored 214 with the Jacobian tempered 150
  lr26_tempered           434 / 475 / 1      9, 6      434 / 475    0 / 0        decisions with T ignored 221 with the Jacobian tempered 216
  lr7_tempered            379 / 528 / 3      19, 14    379 / 528    0 / 0        decisions with T ignored 189 with the Jacobian tempered 163
  rosenbrock7_tempered    295 / 614 / 1      6, 9      22 / 48      273 / 566    decisions with T ignored 125 with the Jacobian tempered 83
  prog_mvn2               281 / 627 / 2      83, 69    24 / 46      257 / 581
  prog_mvn3               274 / 632 / 4      47, 49    22 / 47      252 / 585
  prog_mvn32              146 / 762 / 2      9, 10     15 / 55      131 / 707
  rosenbrock32            326 / 583 / 1      11, 7     24 / 46      302 / 537
  mvn8_n1_rows3           6 / 6 / 28         0, 0      1 / 2        5 / 4
  mvn8_n2_rows3           21 / 42 / 17       4, 1      11 / 11      10 / 31
  mvn8_n1                 5 / 35 / 0         1, 2      0 / 13       5 / 22
  mvn8_n63                661 / 1850 / 9     66, 64    204 / 613    457 / 1237
  mvn8_n64                648 / 1907 / 5     73, 68    203 / 627    445 / 1280
  mvn8_n65                583 / 2006 / 11    54, 44    177 / 665    406 / 1341
  mvn8_n129               1330 / 3823 / 7    123, 130  406 / 1271   924 / 2552
  mvn7_n1_rows3           12 / 23 / 5        0, 0      6 / 6        6 / 17
  mvn7_n2_rows3           20 / 25 / 35       0, 0      4 / 9        16 / 16
  mvn7_n1                 12 / 28 / 0        0, 0      4 / 9        8 / 19
  mvn7_n63                656 / 1856 / 8     67, 70    206 / 612    450 / 1244
  mvn7_n64                644 / 1905 / 11    75, 61    188 / 642    456 / 1263
  mvn7_n65                711 / 1881 / 8     78, 78    212 / 631    499 / 1250
  mvn7_n129               1363 / 3789 / 8    157, 136  425 / 1249   938 / 2540
  mvn5_k1                 859 / 1928 / 13    126, 100  859 / 1928   0 / 0
  mvn7_k1                 775 / 2014 / 11    76, 80    775 / 2014   0 / 0
  mvn5_never              0 / 0 / 0          0, 0      0 / 0        0 / 0
  mvn5_every_k_plus_1     57 / 152 / 1       5, 6      0 / 0        57 / 152
  mvn7_every_k_plus_1     186 / 509 / 5      20, 15    63 / 146     123 / 363
  rosenbrock7_own_row     645 / 2149 / 6     12, 10    42 / 237     603 / 1912
  mvn8_own_row            663 / 2132 / 5     67, 48    58 / 220     605 / 1912
  mvn10_own_row           689 / 2106 / 5     52, 64    79 / 201     610 / 1905
  mvn8_inf                223 / 665 / 22     17, 16    223 / 665    0 / 0
  mvn10_inf               203 / 687 / 20     13, 14    203 / 687    0 / 0
  mvn7_gamma_point        214 / 694 / 2      16, 15    19 / 51      195 / 643
  mvn8_gamma_point        207 / 701 / 2      19, 15    207 / 701    0 / 0
(rosenbrock32, prog_mvn32 and lr26_tempered miss the exponent condition with the overdispersion of their kind -- flips 0 and 3, 6 and
2, 0 and 7 -- and start at a quarter, a half and a half of it.)"""
import zlib

import numpy as np

import demc_jl_amd as demc
import snooker_reference as sr
from program_texts import ROSENBROCK, box_closure, box_program, mvn_program, rosenbrock_closure

N, G = 70, 40
GAMMA_S = (1.2, 2.2)
LR_NOBS = 40
WINDOW_BS = 64          # chains of a workgroup (one wave) of the one-lane kernels


def _seed(name):
    return 20261020 + zlib.crc32(name.encode()) % 100000


def _problem(kind, d, name, m_arch=40, n=N, spread=1.0):
    """target / closure, Z0 (m_arch archive-only rows, then the n starting states; spread: their overdispersion against the other
    worlds of the kind), eps, gamma"""
    r = np.random.default_rng(_seed(name))
    M0 = m_arch + n
    nrm = r.standard_normal((M0, d))
    if kind in ("mvn", "prog_mvn"):
        w = demc.workloads.mvnormal_problem(d, n)
        Z0 = w["mu"] + (2.0 * spread) * nrm @ np.linalg.cholesky(w["Sigma"]).T
        t = w["target"]
        if kind == "prog_mvn":      # the device runs the program, the reference the oracle's built-in log-density
            return dict(target=mvn_program(t.mu, t.W, t.c0), ref_target=t, closure=None, Z0=Z0, eps=w["eps_scale"], gamma=w["gamma"])
        return dict(target=t, closure=None, Z0=Z0, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "iso":
        w = demc.workloads.iso_quad_problem(d, n)
        return dict(target=w["target"], closure=None, Z0=w["mu"] + spread * nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "lr":
        w = demc.workloads.linreg_problem(d, n, nobs=LR_NOBS)
        return dict(target=w["target"], closure=None, Z0=w["beta"] + (0.3 * spread) * nrm, eps=w["eps_scale"], gamma=w["gamma"])
    if kind == "rosenbrock":
        return dict(target=demc.ProgramTarget(ROSENBROCK, d), closure=rosenbrock_closure, Z0=(0.5 * spread) * nrm + 0.5, eps=1e-3 * np.ones(d), gamma=0.5)
    if kind == "box":               # bounded support: -inf outside |x_i| <= 1.5
        c, h = np.zeros(d), 1.5 * np.ones(d)
        return dict(target=box_program(c, h), closure=box_closure(c, h), Z0=0.8 * nrm, eps=1e-3 * np.ones(d), gamma=1.0)
    raise ValueError(kind)


def temperatures():
    """hot, cold, zero, huge, tiny in turn: with snooker generations every 3 each of them meets snooker and ordinary generations"""
    return np.array([(10.0, 0.25, 0.0, 1e300, 1e-300)[g % 5] for g in range(G)])


#        name               kind          d   K  every  more
WORLDS = {
    "mvn2":           ("mvn", 2, 3, 3, {}),
    "mvn5":           ("mvn", 5, 10, 10, {}),
    "mvn5_all":       ("mvn", 5, 3, 1, {}),                       # every generation of a whole run is a snooker generation
    "mvn7":           ("mvn", 7, 10, 3, {}),
    "mvn20":          ("mvn", 20, 3, 3, {}),
    "mvn33":          ("mvn", 33, 10, 1, {}),
    "iso10":          ("iso", 10, 10, 3, {}),
    "iso6":           ("iso", 6, 3, 1, {}),
    "lr10":           ("lr", 10, 3, 3, {}),
    "lr4":            ("lr", 4, 10, 10, {}),
    "rosenbrock7":    ("rosenbrock", 7, 10, 3, {}),
    "box4":           ("box", 4, 3, 3, {}),
    "mvn6_blocks":    ("mvn", 6, 10, 3, dict(blocks=[[0, 1], [2, 3], [4, 5]])),
    "mvn5_tempered":  ("mvn", 5, 10, 3, dict(tempered=True)),
    "mvn5_own_row":   ("mvn", 5, 10, 1, dict(m_arch=3, needs_invalid=True)),
    "iso6_inf":       ("iso", 6, 3, 3, dict(inf_rows=True, needs_invalid=True)),
}

_TEMPERED = dict(tempered=True, plain_piece=True)      # temperatures, and one piece of the schedule without them
_HALVES = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]
NEW_WORLDS = {
    "mvn3":           ("mvn", 3, 3, 3, {}),                       # the specialisations no test had launched
    "mvn4":           ("mvn", 4, 10, 3, {}),
    "mvn8":           ("mvn", 8, 3, 3, {}),
    "mvn10":          ("mvn", 10, 10, 3, {}),                     # (the largest d with W in scalar registers)
    "lr26":           ("lr", 26, 3, 3, {}),
    "lr7":            ("lr", 7, 3, 3, {}),                        # generic regression at an odd d
    "mvn64_all":      ("mvn", 64, 10, 1, {}),                     # MAX_D: 64 KiB of dynamic LDS.  (every = 3 gives 1 and 2 exponent flips)
    "iso64":          ("iso", 64, 3, 3, {}),
    "mvn10_halves":   ("mvn", 10, 10, 3, dict(blocks=_HALVES)),                                               # grouped, scalar registers
    "mvn20_4x5":      ("mvn", 20, 3, 3, dict(blocks=[list(range(5 * i, 5 * i + 5)) for i in range(4)])),      # grouped, from memory
    "mvn8_inter":     ("mvn", 8, 3, 3, dict(blocks=[[0, 2, 4, 6], [1, 3, 5, 7]])),                            # no grouping: the ungrouped path
    "mvn8_tempered":  ("mvn", 8, 10, 3, _TEMPERED),
    "mvn20_tempered": ("mvn", 20, 10, 3, _TEMPERED),
    "mvn13_tempered": ("mvn", 13, 10, 3, _TEMPERED),
    "mvn10_halves_tempered": ("mvn", 10, 10, 3, dict(_TEMPERED, blocks=_HALVES)),
    "iso10_tempered": ("iso", 10, 3, 3, _TEMPERED),
    "iso6_tempered":  ("iso", 6, 3, 3, _TEMPERED),
    "lr10_tempered":  ("lr", 10, 10, 3, _TEMPERED),
    "lr26_tempered":  ("lr", 26, 3, 3, dict(_TEMPERED, spread=0.5)),       # (spread 1: no step whose decision the exponent d - 2 changes)
    "lr7_tempered":   ("lr", 7, 3, 3, _TEMPERED),
    "rosenbrock7_tempered": ("rosenbrock", 7, 10, 3, _TEMPERED),
    "prog_mvn2":      ("prog_mvn", 2, 10, 3, {}),
    "prog_mvn3":      ("prog_mvn", 3, 10, 3, {}),
    "prog_mvn32":     ("prog_mvn", 32, 10, 3, dict(spread=0.5)),                   # (spread 1: 6 and 2 exponent flips)
    "rosenbrock32":   ("rosenbrock", 32, 10, 3, dict(spread=0.25)),               # straight-line code, no data.  (spread 1: 0 and 3 flips)
}
MAIN = {**WORLDS, **NEW_WORLDS}

_OWN = dict(m_arch=3, needs_invalid=True)
_INF = dict(inf_rows=True, needs_invalid=True)
EDGE_WORLDS = {}
for _d in (8, 7):                                                  # specialised, generic
    EDGE_WORLDS.update({
        f"mvn{_d}_n1_rows3":  ("mvn", _d, 3, 1, dict(N=1, m_arch=2, three_rows=True)),       # draw_anchor multiplies by M - 2 = 1
        f"mvn{_d}_n2_rows3":  ("mvn", _d, 3, 1, dict(N=2, m_arch=1, three_rows=True)),
        f"mvn{_d}_n1":        ("mvn", _d, 3, 1, dict(N=1)),
        **{f"mvn{_d}_n{n}":   ("mvn", _d, 3, 1, dict(N=n)) for n in (63, 64, 65, 129)},      # about the workgroup of 64 chains
    })
EDGE_WORLDS.update({
    "mvn5_k1":            ("mvn", 5, 1, 1, {}),                    # every launch a snooker launch, a boundary and an append
    "mvn7_k1":            ("mvn", 7, 1, 1, {}),
    "mvn5_never":         ("mvn", 5, 10, G + 1, {}),               # every > G: no snooker launch; the handle without set_snooker
    "mvn5_every_k_plus_1": ("mvn", 5, 10, 11, {}),
    "mvn7_every_k_plus_1": ("mvn", 7, 3, 4, {}),
    "rosenbrock7_own_row": ("rosenbrock", 7, 10, 1, _OWN),         # e2 == 0 in front of a (straight-line) program
    "mvn8_own_row":       ("mvn", 8, 10, 1, _OWN),                 # NaN / Inf through the scalar-register whitening
    "mvn10_own_row":      ("mvn", 10, 10, 1, _OWN),
    "mvn8_inf":           ("mvn", 8, 3, 3, _INF),
    "mvn10_inf":          ("mvn", 10, 3, 3, _INF),
    "mvn7_gamma_point":   ("mvn", 7, 10, 3, dict(gamma_s=(1.7, 1.7))),       # gamma_lo == gamma_hi
    "mvn8_gamma_point":   ("mvn", 8, 3, 3, dict(gamma_s=(1.7, 1.7))),
})
ALL = {**MAIN, **EDGE_WORLDS}

# the d each built-in target's one-lane dispatch specialises (snooker_kernel_fn); every other d <= 64 runs the run-time-d form
SPECIALISED = {"mvn": (2, 3, 4, 5, 8, 10, 20), "iso": (10,), "lr": (10, 26)}
TARGET_NAME = {"mvn": "MVNORMAL", "iso": "ISO_QUAD", "lr": "LINREG_SSE"}
PLANNED_NAMES = (
    {f"demcz::snooker_kernel<{TARGET_NAME[k]}, {d}>" for k, ds in SPECIALISED.items() for d in ds}
    | {f"demcz::snooker_kernel_generic<{t}>" for t in TARGET_NAME.values()}
    | {f"demcz::snooker_kernel<4, {d}> (program)" for d in (2, 3, 4, 7, 32)})


def planned_kernel(w):
    """The name demcz_debug_kernel_name gives behind a snooker launch of the world."""
    kind, d = w["kind"], w["d"]
    if kind not in SPECIALISED:
        return f"demcz::snooker_kernel<4, {d}> (program)"
    return f"demcz::snooker_kernel<{TARGET_NAME[kind]}, {d}>" if d in SPECIALISED[kind] else f"demcz::snooker_kernel_generic<{TARGET_NAME[kind]}>"


def snooker_generations(w):
    return [g for g in range(1, w["G"] + 1) if g % w["every"] == 0]


def _cuts(every, g_last):
    """The last generation of every demcz_run call: a call that ends in front of a snooker generation, the call that is (or ends on)
    that generation, one that ends in front of a later one inside a stretch, one that ends on a snooker generation, the rest."""
    sn = [g for g in range(1, g_last + 1) if g % every == 0]
    if not sn:
        return [g_last // 4, g_last // 2 + 1, g_last]
    a = sn[0] if sn[0] > 1 else sn[1]
    return sorted({a - 1, a, sn[len(sn) // 2] - 1, sn[(3 * len(sn)) // 4], g_last})


def world(name):
    kind, d, K, every, more = ALL[name]
    n = more.get("N", N)
    p = _problem(kind, d, name, more.get("m_arch", 40), n, more.get("spread", 1.0))
    Z0 = np.array(p["Z0"], order="F")
    if more.get("inf_rows"):
        Z0[3, 1], Z0[11, 4], Z0[17, 0] = np.inf, -np.inf, np.inf       # archive-only rows
    cuts = _cuts(every, G)
    # the pieces of the schedule (first, last, with temperatures): the third is the plain one of a world that has one
    pieces = [(a + 1, b, bool(more.get("tempered")) and not (more.get("plain_piece") and i == 2)) for i, (a, b) in enumerate(zip([0] + cuts[:-1], cuts))]
    return dict(name=name, kind=kind, d=d, N=n, G=G, K=K, every=every, gamma_s=more.get("gamma_s", GAMMA_S), seed=_seed(name), Z0=Z0,
                blocks=more.get("blocks", [list(range(d))]), temperature=temperatures() if more.get("tempered") else None,
                needs_invalid=bool(more.get("needs_invalid")), three_rows=bool(more.get("three_rows")), target=p["target"],
                ref_target=p.get("ref_target", p["target"]), closure=p["closure"], eps=p["eps"], gamma=p["gamma"], pieces=pieces)


def piece_temperature(w, a, b, tempered):
    return w["temperature"][a - 1:b] if tempered else None


def launches_after(w):
    """Window launches made when each piece has run, by DESIGN.md section 4.15's rule: a launch ends at its call's end, at the next
    multiple of K and in front of the next snooker generation; a snooker generation is a launch of its own."""
    K, every, out, n = w["K"], w["every"], [], 0
    for a, b, _ in w["pieces"]:
        g = a
        while g <= b:
            if g % every == 0:
                end = g
            else:
                end = min(b, -(-g // K) * K, -(-g // every) * every - 1)
            n += 1
            g = end + 1
        out.append(n)
    return out


def mixed_run(O, w, **over):
    """A MixedRun of the world, its options overridden by `over`."""
    kw = dict(N=w["N"], d=w["d"], K=w["K"], G=w["G"], blocks=w["blocks"], eps=w["eps"], seed=w["seed"], Z0=w["Z0"],
              target=None if w["closure"] else w.get("ref_target", w["target"]), closure=w["closure"], every=w["every"], gamma_s=w["gamma_s"])
    kw.update(over)
    return sr.MixedRun(O, **kw)


_REF = {}


def reference(O, name):
    """(world, the reference's result, its MixedRun) of the whole run -- in one piece unless a piece of the world's schedule is a
    plain one; computed once and shared -- do not write to it."""
    if name not in _REF:
        w = world(name)
        run = mixed_run(O, w)
        if w["temperature"] is None or all(t for _, _, t in w["pieces"]):
            run.run(1, w["G"], w["gamma"], w["temperature"])
        else:
            for a, b, t in w["pieces"]:
                run.run(a, b, w["gamma"], piece_temperature(w, a, b, t))
        _REF[name] = (w, run.result(), run)
    return _REF[name]


# (world, append lag in batches of K-windows): a sharded handle with a lag is the one whose snooker kernel stores the boundary
# snapshot (WindowParams::snap) that the batched all-gather turns into archive rows
LAGGED = (("mvn5", 1), ("mvn33", 1), ("iso6", 2))


def lagged_reference(O, name, E):
    """The world under demcz_set_append_lag(E): the rows of boundary j join batch J = ceil(j / E) E and are drawn from generation
    (J + E) K + 1 on; at the end of the run all of them are in the archive, in the order of their boundaries."""
    key = (name, E)
    if key not in _REF:
        w = world(name)
        run = mixed_run(O, w, external=True)
        K, pending = w["K"], []
        for a in range(1, w["G"] + 1, K):
            b = min(a + K - 1, w["G"])
            while pending and pending[0][0] <= a:
                run.append_rows(pending.pop(0)[1])
            run.run(a, b, w["gamma"], None)
            if b % K == 0:
                J = -(-(b // K) // E) * E
                pending.append(((J + E) * K + 1, run.result()["X"]))
        for _, rows in pending:
            run.append_rows(rows)
        _REF[key] = (w, run.result(), run)
    return _REF[key]


# ---- what the reference shows of a world (tests/test_snooker_cases.py asserts on these; scripts print them) -----------------------------
def _accepts(logu, dlt, jac):
    with np.errstate(all="ignore"):
        return bool(np.float64(logu) < np.float64(dlt) + np.float64(jac))


def step_counts(O, w, run):
    """Counts over the snooker steps of a reference run.  A step's decision is redone from its facts with one thing changed: the
    Jacobian's exponent d - 2 or d; the temperature ignored; the Jacobian divided by T with the difference."""
    d, K = w["d"], w["K"]
    c = dict(accepted=0, rejected=0, invalid=0, flip_lo=0, flip_hi=0, b_acc=0, b_rej=0, nb_acc=0, nb_rej=0, t_ignored=0, t_jacobian=0,
             last_wave=set(), part_wave=set(), T_at_snooker=set())
    first_of_last_wave = WINDOW_BS * ((w["N"] - 1) // WINDOW_BS)
    for g, ch, f in run.steps:
        if f["T"] is not None:
            c["T_at_snooker"].add(f["T"])
        if ch >= first_of_last_wave:
            c["last_wave"].add(f["accepted"])
        if ch >= WINDOW_BS:
            c["part_wave"].add(f["accepted"])
        if not f["valid"]:
            c["invalid"] += 1
            continue
        acc = f["accepted"]
        c["accepted" if acc else "rejected"] += 1
        c[("b_" if g % K == 0 else "nb_") + ("acc" if acc else "rej")] += 1
        base = float(O.dm_log(f["f2"])) - float(O.dm_log(f["e2"]))
        assert f["jac"] == (0.5 * float(d - 1)) * base and _accepts(f["logu"], f["dlt"], f["jac"]) == acc
        c["flip_lo"] += _accepts(f["logu"], f["dlt"], (0.5 * float(d - 2)) * base) != acc
        c["flip_hi"] += _accepts(f["logu"], f["dlt"], (0.5 * float(d)) * base) != acc
        if f["T"] is not None:
            with np.errstate(all="ignore"):
                raw = np.float64(f["lp_prop"]) - np.float64(f["lp"])
                both = (raw + np.float64(f["jac"])) / np.float64(f["T"])
                c["t_ignored"] += _accepts(f["logu"], raw, f["jac"]) != acc
                c["t_jacobian"] += bool(np.float64(f["logu"]) < both) != acc
    return c


def grouping_counts(O, w, run):
    """(valid steps, accepted steps) whose proposal has other log-density bits when the quadratic form is summed in one piece."""
    flat = mixed_run(O, w, blocks=[list(range(w["d"]))])
    n = na = 0
    for _, _, f in run.steps:
        if f["valid"] and np.float64(flat.logobj(f["xp"])).tobytes() != np.float64(f["lp_prop"]).tobytes():
            n += 1
            na += f["accepted"]
    return n, na
