"""CPU tier: the worlds of tests/closure_cases.py are worth running -- from the oracle alone.

The closure path has two forms, plain (demcz_accept_commit without a temperature) and tempered, times three call modes that must
not differ.  A bit comparison of the history sees a wrong proposal only where it is accepted, a wrong accept test only on a
realised accept / reject path; the proposals themselves are compared one by one with helpers.oracle_sample_logobj's, accepted
or not.  So:
  * the two references are one: the Python loop around the closure reproduces block_cases.oracle_run's chain, log_obj, Z, M and
    changed counts bit for bit, in every world, tempered pieces included;
  * block outcomes: in every main world with disjoint blocks and 2 <= NB <= 5 every one of the 2^NB outcome vectors of a generation
    occurs at least three times in the plain generations and at least three times in the tempered ones;
  * full-update moves: in the one-block worlds "moved" and "did not move" and each (previous, this) pair occur at least three
    times per form;
  * temperatures matter: every tempered piece depends on its temperatures in at least three chains;
  * the two new worlds (d = 1; d = 33 in one block) meet the three conditions of tests/test_full_update_cases.py;
  * the edge worlds accept and reject (strictly between 0.1 and 0.9; one chain: both outcomes at least three times), the box
    closure returns -inf, NaN and +inf at least three times each.
The table in closure_cases' docstring is what this file prints."""
import numpy as np
import pytest

import block_cases as bc
import closure_cases as cc
from demc_jl_amd.sampler import blocks_per_generation
from helpers import bits_differ

MAIN = list(cc.MAIN_WORLDS)
EDGES = {c["name"]: c for c in cc.edge_cases()}


def test_the_world_lists_are_the_planned_ones():
    assert len(cc.BLOCK_WORLDS) == 21 and len(cc.FULL_WORLDS) == 10 and len(cc.NEW_WORLDS) == 2 and len(set(MAIN)) == 33
    assert {cc.main_case("full_" + w)["d"] for w in cc.FULL_WORLDS if w.startswith("mvn")} == {2, 3, 5, 7, 9, 13, 20, 64}
    dims = {cc.main_case(w)["d"] for w in MAIN}
    assert {1, 2, 3, 33, 64} <= dims and max(dims) == 64                       # 64: (d + 1) * 64 doubles = 33 280 bytes of LDS
    assert (64 + 1) * cc.PROPOSE_BS * 8 == 33280
    for w in MAIN:
        case = cc.main_case(w)
        assert case["K"] == 5 and case["N"] in (96, 64) and case["G"] in (100, 120, 25)
        assert {p[3] for p in case["pieces"]} == set(bc.FORMS), w
    singles = cc.main_case("d5_singles")
    assert all(len(b) == 1 for b in singles["blocks"]) and len(singles["blocks"]) == 5 and singles["G"] == 120
    assert cc.main_case("left_out")["blocks"] == [[0, 1], [3]] and cc.main_case("left_out")["d"] == 5
    many = cc.main_case("many_blocks")
    assert len(many["blocks"]) == 65 and blocks_per_generation(many["blocks"]) == 3 * 33 + 3 * 32
    assert not bc.disjoint(many) and not bc.disjoint(cc.main_case("d20_overlap"))
    # an odd block longer than 3 (the last pair's second normal is unused)
    assert any(len(b) % 2 == 1 and len(b) > 3 for w in MAIN for b in cc.main_case(w)["blocks"])
    assert cc.one_block(cc.main_case("iso1")) and cc.one_block(cc.main_case("mvn33")) and cc.main_case("iso1")["problem"]["mu"].tolist() == [0.0]


def test_the_edge_schedules_are_the_planned_ones():
    alt = cc.pieces_of(cc.ALTERNATE)
    assert len(alt) == 25 and [p[2] for p in alt] == [g % 2 == 1 for g in range(1, 26)] and all(a == b for a, b, _, _ in alt)
    assert [cc.workgroups(N)[0] for N in cc.POPULATIONS] == [1, 1, 1, 2, 3, 4, 4, 5]
    assert [cc.workgroups(N)[1] for N in cc.POPULATIONS] == [1, 1, 1, 1, 1, 1, 1, 2]
    assert {N % cc.PROPOSE_BS for N in cc.POPULATIONS} >= {0, 1, 63} and {N % cc.COMMIT_BS for N in cc.POPULATIONS} >= {0, 1, 255}
    for lengths, G in ((cc.LENGTHS_40, 40), (cc.LENGTHS_41, 41), (cc.LENGTHS_45, 45), (cc.ZERO_LENGTHS, 40)):
        assert cc.pieces_of(lengths)[-1][1] == G
    assert cc.archive_case(1)["K"] == 1 and cc.archive_case(41)["K"] == 41 > cc.archive_case(41)["G"] == 40
    assert cc.ORIGIN % cc.K == 0 and cc.origin_case()["G"] == 2 * cc.ORIGIN + 1 and cc.capacity_case()["G"] % cc.K == 0
    assert cc.SWITCH_AT % cc.K != 0 and cc.switch_case()["G"] > cc.SWITCH_AT
    for case in cc.zero_temperature_cases():
        assert {0.0, 1e-300, 1e300} <= set(case["temperature"].tolist()) and all(p[2] for p in case["pieces"]) and case["G"] == 40
    assert [c["d"] for c in cc.zero_temperature_cases()] == [6, 64] and cc.one_block(cc.zero_temperature_cases()[1])
    assert len(EDGES) == len(cc.edge_cases())                                   # (the references are kept by name)
    assert not set(EDGES) & {cc.main_case(w)["name"] for w in MAIN}


def _same_run(loop, ref, what):
    for k in ("chain", "log_obj", "X", "logp", "Z"):
        why = bits_differ(loop[k], ref[k])
        assert why is None, f"{what}: the loop around the closure against the oracle's run: {k}: {why}"
    assert loop["M"] == ref["M"] and np.array_equal(loop["changed"], ref["changed"]), what


def _xprop_is_consistent(case, loop):
    """A proposal's columns outside its block are the bits of the state the block-step started from; an accepted proposal is the
    next state."""
    x0 = np.array(case["problem"]["Zinit"][-case["N"]:])
    full = np.concatenate([x0[:, :, None], loop["chain"]], axis=2)
    xp = loop["xprop"]
    assert xp.shape == (case["N"], case["d"], case["G"], len(case["blocks"]))
    out0 = [p for p in range(case["d"]) if p not in case["blocks"][0]]
    u = lambda a: np.ascontiguousarray(a).view(np.uint64)      # noqa: E731
    assert (u(xp[:, :, :, 0][:, out0, :]) == u(full[:, out0, :-1])).all()
    last = len(case["blocks"]) - 1
    same_as_next = (u(xp[:, :, :, last]) == u(loop["chain"])).all(axis=1)
    assert same_as_next.any() and not same_as_next.all()


@pytest.mark.parametrize("world", MAIN)
def test_main_worlds_meet_their_conditions(oracle, world):
    case = cc.main_case(world)
    ref = cc.reference(oracle, case)
    loop = cc.proposal_loop(oracle, case)
    _same_run(loop, ref, world)
    _xprop_is_consistent(case, loop)
    NB = len(case["blocks"])
    share = ref["changed"].sum() / (case["N"] * case["G"])
    diffs = bc.untempered_differences(oracle, case, ref)
    assert len(diffs) == sum(1 for p in case["pieces"] if p[2]) >= 1 and min(diffs) >= 3, f"{world}: chains that differ without the temperatures {diffs}"
    if NB == 1:
        outcomes, pairs = cc.plain_tempered(bc.outcome_counts(case, ref)), cc.plain_tempered(bc.pair_counts(case, ref))
        rarest = {t: min(int(outcomes[t].min()), int(pairs[t].min())) for t in outcomes}
        for t in outcomes:
            assert outcomes[t].shape == (2,) and (outcomes[t] >= 3).all(), f"{world}, {t}: moved / did not move {outcomes[t]}"
            assert pairs[t].shape == (1, 2, 2) and (pairs[t] >= 3).all(), f"{world}, {t}: (previous, this) pairs {pairs[t].tolist()}"
    elif bc.disjoint(case) and NB <= 5:
        outcomes = cc.plain_tempered(bc.outcome_counts(case, ref))
        rarest = {t: int(outcomes[t].min()) for t in outcomes}
        for t in outcomes:
            missing = [format(o, "0%db" % NB) for o in range(1 << NB) if outcomes[t][o] < 3]
            assert not missing, f"{world}, {t}: outcome vectors seen fewer than three times: {missing}"
    else:
        assert world in ("d20_overlap", "many_blocks")
        rarest = {}
        assert share > 0.2
    print("%-20s d %2d NB %2d gamma %-5s share moved %.3f | rarest plain %s tempered %s | %d" %
          (world, case["d"], NB, case["gamma"], share, rarest.get("plain", "-"), rarest.get("tempered", "-"), min(diffs)))
    if world in cc.NEW_WORLDS:
        # the three conditions of tests/test_full_update_cases.py, per finer form
        o4, p4 = bc.outcome_counts(case, ref), bc.pair_counts(case, ref)
        for form in bc.FORMS:
            assert (o4[form] >= 3).all() and (p4[form] >= 3).all(), f"{world}, {form}: {o4[form]}, {p4[form].tolist()}"
        assert 0.25 <= share <= 0.75, f"{world}: a chain moves in {share:.3f} of its generations"
        print("%-20s rarest pair over the four forms %d" % (world, min(int(p4[f].min()) for f in bc.FORMS)))


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_worlds_accept_and_reject(oracle, name):
    case = EDGES[name]
    ref = cc.reference(oracle, case)
    loop = cc.proposal_loop(oracle, case)
    _same_run(loop, ref, name)
    _xprop_is_consistent(case, loop)
    acc = ref["changed"].sum() / (case["N"] * case["G"])
    print("%-40s N %3d G %2d acceptance %.3f" % (name, case["N"], case["G"], acc))
    if name == "closure_box":
        kinds = cc.box_kinds(loop["proposed"])
        print("%-40s proposals at -inf, NaN, +inf: %s of %d" % (name, kinds, loop["proposed"].size))
        assert min(kinds) >= 3
        x0 = case["problem"]["Zinit"][-case["N"]:]
        assert np.isfinite([cc.box_closure(list(map(float, r))) for r in x0]).all(), "the start is inside the box"
        assert np.isposinf(ref["logp"]).sum() >= 1 and np.isfinite(ref["logp"]).sum() >= 3       # a chain at +inf stays there
    elif "zero_temperature" in name:
        assert acc > 0.1                                   # (T = 0 accepts every improvement and nothing else)
    elif case["N"] == 1:
        moved = ref["changed"]
        assert (moved == 1).sum() >= 3 and (moved == 0).sum() >= 3, moved
    else:
        assert 0.1 < acc < 0.9, f"{name}: acceptance {acc:.3f}"


def test_the_archive_edges_append_as_planned(oracle):
    k1, k41 = cc.archive_case(1), cc.archive_case(41)
    M0 = k1["problem"]["Zinit"].shape[0]
    assert cc.reference(oracle, k1)["M"] == M0 + k1["N"] * 40 and cc.reference(oracle, k41)["M"] == M0
    cap = cc.capacity_case()
    assert cc.reference(oracle, cap)["M"] == M0 + cap["N"] * 9
    assert cc.rng_offset_case()["rng_offset"] == 7
