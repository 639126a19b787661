"""Without a GPU: the worlds of tests/bridge_cases.py through the two restatements of the iteration (tests/bridge_reference.py).

  * the tolerances the device is held to are ten times the measured error of the float64 restatement against the wide one; the
    measurements are printed, and the restatement is held to a tenth of each constant;
  * in every converging world the wide reference's last change is <= tol / 4 and the one before it >= 4 tol, so that the update
    count does not hang on the last bits of an exp;
  * the worlds that must give NaN give NaN in both, with the NaN count of a2;
  * the host arithmetic of demc.bayes_factor and demc.post_prob, and ProgramTarget.check_bridge, which needs no device."""
import math

import numpy as np
import pytest

import bridge_cases as bc
import bridge_reference as br
import program_texts as pt

WORLDS = list(range(len(bc.worlds())))
IDS = bc.names()


def test_the_cases_the_issue_lists_are_there():
    w = {x["name"]: x for x in bc.worlds()}
    assert np.mean(np.isneginf(w["half_outside"]["a2"])) > 0.3
    assert w["more_proposal"]["a2"].size != w["more_proposal"]["a1"].size != w["fewer_proposal"]["a2"].size
    assert w["neff_seventh"]["args"]["neff"] == w["neff_seventh"]["a1"].size / 7.0
    assert np.isnan(w["nan_in_a2"]["a2"]).sum() == 3 and w["max_iter_3"]["args"]["max_iter"] == 3
    assert all(x["a1"].size <= 5000 and x["a2"].size <= 5000 for x in w.values())
    assert abs(bc.reference(IDS.index("offset_plus"))["logml"] - 1e4) < 10 and abs(bc.reference(IDS.index("offset_minus"))["logml"] + 1e4) < 10


@pytest.mark.parametrize("i", WORLDS, ids=IDS)
def test_world_conditions(i):
    w, ref = bc.worlds()[i], bc.reference(i)
    tol = w["args"]["tol"]
    if w["nan"]:
        assert math.isnan(ref["logml"]) and not ref["converged"] and ref["f2"] is None
        return
    d = ref["deltas"]
    print(f"[bridge] {w['name']}: changes {' '.join(f'{x:.1e}' for x in d)} (tol {tol:.0e})")
    if w["converges"]:
        assert ref["converged"] and 2 <= ref["iterations"] <= 12
        assert d[-1] <= tol / 4.0 and d[-2] >= 4.0 * tol
    else:
        assert not ref["converged"] and ref["iterations"] == w["args"]["max_iter"] and d[-1] >= 4.0 * tol


def test_restatement_against_the_wide_reference():
    worst = dict(logml=(0.0, ""), moments=(0.0, ""), se=(0.0, ""), f2=(0.0, ""))
    for i, w in enumerate(bc.worlds()):
        ref, f = bc.reference(i), bc.restatement(i)
        assert f["n_nan"] == ref["n_nan"] == int(np.isnan(w["a2"]).sum())
        assert f["converged"] == ref["converged"] and f["iterations"] == ref["iterations"]
        if w["nan"]:
            assert math.isnan(f["logml"]) and np.all(np.isnan(f["moments"]))
            continue
        e = br.errors(f, ref)
        se_ref, ess, _ = bc.reference_se(i)
        e["se"] = abs(br.se_of(f["moments"], w["a2"].size, ess) - se_ref) / se_ref
        e["f2"] = float(np.max(np.abs(f["f2"] - ref["f2"]) / ref["f2"]))
        for k, v in e.items():
            if v > worst[k][0]:
                worst[k] = (v, w["name"])
    for k, tol in (("logml", br.LOGML_TOL), ("moments", br.MOMENT_TOL), ("se", br.SE_TOL), ("f2", br.F2_TOL)):
        print(f"[bridge] float64 restatement against the wide reference: {k} {worst[k][0]:.3e} ({worst[k][1]}); tolerance {tol:.1e}")
        assert worst[k][0] <= tol / 10.0 * 1.0001 and tol <= 10.0 * worst[k][0] * 1.06         # (the constant is 10 x the measurement)


def test_bayes_factor_and_post_prob(demc):
    B = lambda lm, se: demc.Bridge(lm, se, 4, True, 10, 10, 10.0, 0, 10.0, None, None)      # noqa: E731
    a, b, c = B(-10.0, 0.03), B(-12.0, 0.04), B(-1e4, 0.1)
    lbf, se = demc.bayes_factor(a, b)
    assert lbf == 2.0 and se == math.sqrt(0.03 ** 2 + 0.04 ** 2)
    p = demc.post_prob(a, b)
    assert np.allclose(p, [1.0 / (1.0 + math.exp(-2.0)), 1.0 / (1.0 + math.exp(2.0))], rtol=1e-15) and abs(p.sum() - 1.0) < 1e-15
    p = demc.post_prob(a, b, c, prior=[1.0, math.exp(2.0), 1.0])
    assert np.allclose(p, [0.5, 0.5, 0.0], atol=1e-15)                  # (a model 1e4 below the others underflows to 0, no NaN)
    assert np.allclose(demc.post_prob(-1e4, -1e4 - math.log(3.0)), [0.75, 0.25], rtol=1e-12)
    assert np.all(np.isnan(demc.post_prob(a, B(float("nan"), 0.0))))
    with pytest.raises(ValueError):
        demc.post_prob(a, b, prior=[1.0])
    assert demc.bridge_seed(5) == 5 ^ demc.BRIDGE_SEED_XOR and demc.bridge_seed(5) != 5
    assert demc.bridge_se([0.5, 0.01, 0.25, 0.02], 100, 50.0) == math.sqrt(0.01 / (100 * 0.25) + 0.02 / (50.0 * 0.0625))


def test_check_bridge_needs_no_device(demc):
    pt.iso_program(np.zeros(3)).check_bridge()
    pt.box_program(np.zeros(2), np.ones(2)).check_bridge()
    with pytest.raises(demc.DemczError) as ei:
        demc.ProgramTarget(pt.SYNTAX_ERROR, 3).check_bridge()
    assert ei.value.code == 1 and "undefined_thing" in str(ei.value) and "program target" in str(ei.value)
    with pytest.raises(demc.DemczError) as ei:
        demc.ProgramTarget("__device__ double f(const double* x) { return x[0]; }", 2).check_bridge()
    assert "demcz_logobj" in str(ei.value)
    with pytest.raises(demc.DemczError):
        demc.ProgramTarget(pt.ISO, 33, data=np.zeros(33)).check_bridge()
