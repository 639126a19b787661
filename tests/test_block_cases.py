"""CPU tier: the worlds of tests/block_cases.py are worth running -- from the oracle alone.

A bit comparison sees a wrong candidate, a wrong group sum or a stale cached partial of the incremental form (Pc / Qc, kept across
block-steps and committed on accept; a rejected candidate leaves no trace in the history) only on a realised accept / reject path.
So the oracle's run of every world must satisfy, per form (the generations of the pieces that run it):
  * the outcome condition: a block-step's outcome is "a parameter of the block differs from the generation before" (disjoint
    blocks, eps > 0).  With at most five blocks every one of the 2^NB outcome vectors of a generation occurs at least three
    times; with more, every block is accepted and rejected at least three times and all four (previous block-step's outcome, this
    one's) pairs occur for every block, the wrap from a generation's last block to block 0 of the next included.  The two worlds
    whose blocks overlap have no such reading of the history: a chain must move in more than 0.2 of its generations, and with
    two blocks in at most 0.999 of them;
  * temperatures matter: every tempered piece, run again by the oracle from the state at its start WITHOUT temperatures, gives a
    different history for at least three chains -- otherwise a kernel that ignored the temperature would pass.
The schedules must plan what they claim by the launch rules in block_cases' docstring, and the instantiations they plan must be
all 31 of window_kernel_mlb that demcz_capi.hip's mlb_kernel can return."""
import numpy as np
import pytest

import block_cases as bc

WORLDS = [("mlb", n) for n in bc.MLB_WORLDS] + [("one", n) for n in bc.ONE_LANE_WORLDS] + [("many", "d10_65_blocks")] + \
         [("four", n) for n in bc.FOUR_WAVE_WORLDS]


def _case(group, name):
    if group == "four":
        return bc.four_wave_case(*name)
    return {"mlb": bc.mlb_case, "one": bc.one_lane_case}[group](name) if group != "many" else bc.many_blocks_case()


@pytest.mark.parametrize("rounds", [2, 4])
def test_the_schedule_tiles_the_run_and_plans_every_form(rounds):
    pieces, K = bc.schedule(rounds), bc.K
    assert pieces[0][0] == 1 and all(a == b + 1 for (_, b, _, _), (a, _, _, _) in zip(pieces, pieces[1:]))
    assert {p[3] for p in pieces} == set(bc.FORMS)
    before = K                                              # (a first call has no draws prepared for it)
    for a, b, tempered, form in pieces:
        assert form.endswith("tempered" if tempered else "plain")
        if form.startswith("LIVE"):
            assert (b - 1) // K > (a - 1) // K + 1          # crosses boundaries
            assert before < K                               # one launch: nothing prepared that would cut it
            assert (a - 1) % K != 0 and b % K == 0          # starts inside a window, ends with one
        else:
            assert (a - 1) // K == (b - 1) // K             # inside one K-window
        before = b - a + 1
    for form in bc.FORMS:
        assert sum(b - a + 1 for a, b, _, f in pieces if f == form) >= (30 if rounds == 4 and "non" in form else 20), form
    cuts = {((a - 1) % K, b - a + 1) for a, b, _, f in pieces if f.startswith("non")}
    assert {(0, 5), (0, 2), (2, 3), (0, 3), (3, 2)} <= cuts       # whole windows and windows cut in two


def test_the_edge_schedules_plan_every_form():
    for lengths in (bc.EDGE_LENGTHS,):
        assert {p[3] for p in bc.pieces_of(lengths)} == set(bc.FORMS)
    T = bc.zero_temperature_case("d10_four")
    assert {0.0, 1e-300, 1e300} <= set(T["temperature"].tolist()) and all(p[2] for p in T["pieces"])
    assert {p[3] for p in T["pieces"]} == {bc.LIVE_TEMPERED, bc.SHORT_TEMPERED}
    r = bc.resumed_case("d20_4x5")
    assert r["pieces"][1][1] == bc.RESUME_AT and bc.RESUME_AT % bc.K != 0
    assert {p[3] for p in r["pieces"]} == set(bc.FORMS)


def test_grouped_restates_the_librarys_rule():
    assert bc.grouped(5, [[0, 1], [2, 3, 4]]) and bc.grouped(6, [[0], [1, 2], [5, 3, 4]]) and bc.grouped(64, [list(range(63)), [63]])
    assert not bc.grouped(5, [[3], [0], [4], [1], [2]]) and not bc.grouped(6, [[0, 2, 4], [1, 3, 5]])
    assert not bc.grouped(10, [[9, 0], [1, 8, 2], [3, 4, 5, 6, 7]])
    assert not bc.grouped(20, [list(range(20)), list(range(5))]) and not bc.grouped(5, [[0, 1], [3]])      # overlap; a parameter left out
    assert not bc.grouped(5, [[0, 1], [2, 3, 4]], kind="iso")
    assert bc.incremental(20, bc.FOUR_BY_FIVE) and not bc.incremental(20, bc.FOUR_BY_FIVE, ("DEMCZ_NO_MLB_INCREMENTAL",))
    assert len(bc.MANY_BLOCKS) == bc.MLB_MAX_BLOCKS + 1 and max(len(b) for b in bc.MANY_BLOCKS) == 2


def test_every_instantiation_is_planned():
    """mlb_kernel / mlb_fn: (D, L) = (5, 8), (6, 8), (10, 8), (20, 16) x {fused, split, split LIVE} x {ungrouped, GM}; QB = 5 fused,
    split, split LIVE; (20, 32) split x LIVE x GM."""
    want = {(d, L, rec, live, 0, gm) for d, L in ((5, 8), (6, 8), (10, 8), (20, 16)) for rec, live in ((False, False), (True, False), (True, True))
            for gm in (False, True)}
    want |= {(20, 16, rec, live, 5, False) for rec, live in ((False, False), (True, False), (True, True))}
    want |= {(20, 32, True, live, 0, gm) for live in (False, True) for gm in (False, True)}
    assert len(want) == 31
    got = bc.instantiations_planned()
    assert got == want, (sorted(want - got), sorted(got - want))
    names = bc.kernel_names_planned()
    # window_kernel_of's table, as demcz_debug_kernel_name spells it
    mlb = {"demcz::window_kernel_mlb<MVNORMAL, %d, %d>" % dl for dl in ((5, 8), (6, 8), (10, 8), (20, 16))}
    mlb |= {"demcz::window_kernel_mlb<MVNORMAL, %d, %d, true, %s>" % (d, L, lv) for d, L in ((5, 8), (6, 8), (10, 8), (20, 16), (20, 32))
            for lv in ("true", "false")}
    mlb |= {"demcz::window_kernel_mlb<MVNORMAL, 20, 16, true, %s, 5>" % lv for lv in ("true", "false")}
    one = {"demcz::window_kernel<MVNORMAL, %d, false>" % d for d in (2, 3, 4, 5, 8, 10, 20, 7, 13, 64)}
    one |= {"demcz::window_kernel<ISO_QUAD, 10, false>", "demcz::window_kernel<ISO_QUAD, 7, false>", "demcz::window_kernel<4, 7, false> (program)"}
    one |= {"demcz::window_kernel<LINREG_SSE, %d, false>" % d for d in (10, 26, 7)}
    assert names == mlb | one, sorted(names ^ (mlb | one))
    # the ten one-lane specialisations, each MvNormal one on both of its run-time paths; the generic kernel for three targets
    spec = {(k, d): set() for k, d, _, _ in bc.ONE_LANE_WORLDS.values()}
    for k, d, blocks, _ in bc.ONE_LANE_WORLDS.values():
        spec[k, d].add(bc.grouped(d, blocks, k))
    assert sum(bc.one_lane_specialised(k, d) for k, d in spec) == 10
    assert all(spec[k, d] == {False, True} for k, d in spec if k == "mvn" and d != 7)
    assert {k for k, d in spec if not bc.one_lane_specialised(k, d)} == {"mvn", "iso", "lr", "prog"}


def test_outcome_counts_read_the_history():
    """Two chains, two blocks, three generations in one non-LIVE piece."""
    case = dict(blocks=[[0], [1, 2]], pieces=[(1, 3, False, bc.SHORT_PLAIN)])
    X0 = np.zeros((2, 3))
    chain = np.zeros((2, 3, 3))
    chain[0, 0, 0:] = 1.0                   # chain 0: block 0 moves in generation 1
    chain[0, 2, 2] = 5.0                    # ... block 1 in generation 3
    chain[1, :, 1:] = 2.0                   # chain 1: both blocks move in generation 2
    ref = dict(X0=X0, chain=chain)
    assert bc.outcome_counts(case, ref)[bc.SHORT_PLAIN].tolist() == [3, 1, 1, 1]
    p = bc.pair_counts(case, ref)[bc.SHORT_PLAIN]
    # block-steps in order: chain 0: 1 0 | 0 0 | 0 1, chain 1: 0 0 | 1 1 | 0 0; the first block-step of the run has none before it
    assert p[1].tolist() == [[3, 1], [1, 1]] and p[0].tolist() == [[2, 1], [1, 0]]


@pytest.mark.parametrize("group,name", WORLDS)
def test_every_block_outcome_occurs_and_temperatures_matter(oracle, group, name):
    case = _case(group, name)
    ref = bc.oracle_run(oracle, case)
    forms = {p[3] for p in case["pieces"]}
    assert forms == set(bc.FORMS) or group == "four"
    acc = ref["changed"].sum() / (case["N"] * case["G"])
    NB = len(case["blocks"])
    if not bc.disjoint(case):
        assert name in ("d20_overlap", "d10_65_blocks")
        print(name, "overlapping blocks: a chain moves in %.3f of its generations" % acc)
        assert acc > 0.2 and (acc <= 0.999 or NB > 5)      # (65 block-steps: some block moves in every generation)
    elif NB <= 5:
        counts = bc.outcome_counts(case, ref)
        print(name, "gamma", case["gamma"], "acceptance %.3f" % acc, "rarest outcome per form", {f: int(counts[f].min()) for f in sorted(forms)})
        for form in forms:
            missing = [format(o, "0%db" % NB) for o in range(1 << NB) if counts[form][o] < 3]
            assert not missing, f"{name}, {form}: outcome vectors seen fewer than three times: {missing}"
    else:
        pairs = bc.pair_counts(case, ref)
        for form in forms:
            p = pairs[form]
            assert (p.sum(axis=1) >= 3).all(), f"{name}, {form}: a block accepted or rejected fewer than three times"
            assert (p >= 1).all(), f"{name}, {form}: a (previous, this) pair of outcomes never seen"
    diffs = bc.untempered_differences(oracle, case, ref)
    assert len(diffs) == sum(1 for p in case["pieces"] if p[2]) >= 1
    print(name, "chains that differ without the temperatures, per tempered piece:", diffs)
    assert min(diffs) >= 3, f"{name}: a tempered piece in which the temperatures change fewer than three chains: {diffs}"


def test_the_left_out_parameters_never_move_in_the_oracle(oracle):
    case = bc.left_out_case()
    ref = bc.oracle_run(oracle, case)
    for p in (2, 4):
        assert (ref["chain"][:, p, :].view(np.uint64) == ref["X0"][:, p, None].view(np.uint64)).all()
    assert (ref["chain"][:, 0, -1] != ref["X0"][:, 0]).sum() > case["N"] // 2


def test_four_wave_populations_fill_the_last_workgroup_partly():
    for name, sign in bc.FOUR_WAVE_WORLDS:
        case = bc.four_wave_case(name, sign)
        L = bc.MLB_LANES[case["d"]]
        assert bc.chain_waves(case) >= 4 * bc.MI355X_CUS                     # demcz_create: four-wave workgroups
        assert case["N"] % (4 * (64 // L)) != 0 and case["N"] % (64 // L) != 0
        assert -(-case["N"] // (4 * (64 // L))) == bc.MI355X_CUS + (sign > 0)    # workgroups: one per CU, or one more
        assert case["G"] == 2 * bc.K + 3 and [p[3] for p in case["pieces"]] == [bc.SHORT_TEMPERED, bc.LIVE_PLAIN]
    assert {bc.MLB_LANES[bc.MLB_WORLDS[n][0]] for n, _ in bc.FOUR_WAVE_WORLDS} == {8, 16}
    assert set(bc.FOUR_WAVE_LIVE) <= set(bc.FOUR_WAVE_WORLDS) and {bc.MLB_LANES[bc.MLB_WORLDS[n][0]] for n, _ in bc.FOUR_WAVE_LIVE} == {8, 16}
    assert bc.per_window_launches(bc.pieces_of([(3, True), (10, False)])) == [1, 4]
