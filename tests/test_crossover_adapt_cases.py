"""CPU: the worlds of tests/crossover_adapt_cases.py are held to their conditions by the reference alone, so that the bit comparison
on the device (tests/test_gpu_crossover_adapt.py, _forms.py) exercises what it is meant to: several updates, weights that move,
class draws that the moved weights change, the floor, the clamp, a column that does not count, accepted steps that add nothing."""
import pytest

import crossover_adapt_cases as ac
import crossover_adapt_reference as ar
import crossover_cases as cc


@pytest.mark.parametrize("name", list(ac.WORLDS))
def test_every_world_updates_and_its_weights_move(oracle, name):
    w, _, run = ac.reference(oracle, name)
    redrawn = ac.redrawn_classes(oracle, run)
    print(name, "updates", run.updates, "changed", ac.changed_updates(run), "redrawn", redrawn, "weights", run.weights, "tried", run.tried)
    assert w["N"] % 64 != 0 and w["N"] > 64 and 40 <= w["N"] <= 130
    assert run.updates >= 3 and run.updates == w["adapt_until"] // w["adapt_every"]
    assert ac.changed_updates(run) >= 2
    assert redrawn >= 1
    assert sum(run.tried) == w["N"] * sum(g <= w["adapt_until"] for g in run.crossover_generations)
    assert 1 <= sum(run.weights) < 2 ** 31 and min(run.weights) >= w["min_weight"]
    # frozen behind `until`
    assert all(run.weights_at[g] == run.weights for g in range(w["adapt_until"] + 1, w["G"] + 1))


@pytest.mark.parametrize("name", list(ac.FORM_WORLDS))
def test_every_form_world_updates_three_times(oracle, name):
    w, _, run = ac.reference(oracle, name)
    print(name, "updates", run.updates, "changed", ac.changed_updates(run), "weights", run.weights)
    assert w["N"] % 64 != 0 and w["N"] > 64
    assert run.updates == 3 and ac.changed_updates(run) >= 2 and ac.redrawn_classes(oracle, run) >= 1


def test_a_world_ends_with_a_class_at_the_floor(oracle):
    w, _, run = ac.reference(oracle, "mvn64_floor")
    print(run.weights, run.update_log[-1])
    assert w["min_weight"] in run.weights and max(run.weights) > w["min_weight"]


def test_a_far_start_clamps_steps(oracle):
    _, _, run = ac.reference(oracle, "mvn5_far")
    print("clamped", ac.clamped_steps(run), "of", len(run.jumps))
    assert ac.clamped_steps(run) >= 10
    assert any(q == int(ar.Q_ONE * ar.Q_ONE) for *_, q in run.jumps)


def test_a_constant_column_does_not_count_in_its_first_period(oracle):
    w, _, run = ac.reference(oracle, "iso10_const")
    col = ac.ALL["iso10_const"][2]["const_col"]
    first_rsd = run.update_log[0][3]
    print("rsd of the first period", first_rsd, "zero-q steps", ac.zero_q_steps(run))
    assert first_rsd[col] == 0.0 and all(v > 0.0 for p, v in enumerate(first_rsd) if p != col)
    assert run.update_log[1][3][col] > 0.0           # the column has moved by the first update
    assert ac.zero_q_steps(run) >= 1                 # accepted steps that moved that column alone add nothing


def test_tempered_worlds_decide_differently(oracle):
    for name in [n for n, v in ac.ALL.items() if v[2].get("tempered")]:
        _, _, run = ac.reference(oracle, name)
        print(name, cc.tempered_flips(run))
        assert cc.tempered_flips(run) >= 10, name


def test_snooker_generations_stand_on_update_positions(oracle):
    w, _, run = ac.reference(oracle, "mvn5_snooker")
    on = [g for g in run.snooker_generations if g % w["adapt_every"] == 0 and g <= w["adapt_until"]]
    assert len(on) >= 3 and run.updates == w["adapt_until"] // w["adapt_every"]


def test_the_new_unit_is_a_source_of_the_library():
    import demc_jl_amd._lib as L
    assert any(p.name == "demcz_crossover_adapt_inst.hip" for p in L.sources())
