"""Every world of tests/loo_cases.py meets the condition it was built for, by the reference alone (tests/loo_reference.py): the
device is then run over worlds that are known to take every path of demcz_kernels_loo.h."""
import math

import numpy as np

import loo_cases as lc
import loo_reference as lr


def _by_name():
    return {w["name"]: i for i, w in enumerate(lc.worlds())}


def test_required_worlds_are_present():
    names = _by_name()
    for need in ("tail4", "tail5", "tail255", "tail256", "tail257", "many_candidates", "low_accept", "poisoned", "heavy_light",
                 "far_from_zero", "floor_cut", "r_eff", "columns1", "columns32", "columns33", "columns70", "window"):
        assert need in names
    shapes = {w["name"]: w["loglik"].shape for w in lc.worlds()}
    assert [shapes[f"columns{n}"][1] for n in (1, 32, 33, 70)] == [1, 32, 33, 70]
    assert max(s[0] * s[1] * s[2] for s in shapes.values()) <= 2e5 * 70


def test_tail_cap_arithmetic():
    assert lr.tail_cap(400) == 60 and lr.tail_cap(8000) == 269 and lr.tail_cap(168000) == 1230
    assert lr.tail_cap(1) == 0 and lr.tail_cap(2) == 1
    assert lr.tail_cap(100, 0.25) == 20 and lr.tail_cap(10000, 4.0) == 150
    assert lr.candidates(5) == 32 and lr.candidates(1225) == 65 and lr.quartile(5) == 1 and lr.quartile(6) == 2


def test_every_world_meets_its_condition():
    seen = set()
    for i, w in enumerate(lc.worlds()):
        ref = lc.reference(i)
        a = lc.window_of(w)
        S = a.shape[0] * a.shape[2]
        for col, want in w["expect"].items():
            r = np.broadcast_to(np.asarray(1.0 if w["r_eff"] is None else w["r_eff"]), (a.shape[1],))[col]
            M = lr.tail_cap(S, float(r))
            for key, val in want.items():
                seen.add(key)
                if key == "n_tail":
                    assert ref["n_tail"][col] == val, w["name"]
                elif key == "no_fit":
                    assert (ref["pareto_k"][col] == math.inf) == val, w["name"]
                elif key == "m_min":
                    assert lr.candidates(int(ref["n_tail"][col])) >= val, w["name"]
                elif key == "n_below_M":
                    assert lr.MIN_FIT <= ref["n_tail"][col] < M, (w["name"], ref["n_tail"][col], M)
                    srt = np.sort(a[:, col, :].ravel())
                    assert srt[M] == srt[M - 1] == srt[ref["n_tail"][col]], "the cutoff is not inside a run of ties"
                elif key == "floor":
                    srt = np.sort(a[:, col, :].ravel())
                    assert srt[0] - srt[M] < lr.LOG_DBL_MIN and ref["n_tail"][col] == np.count_nonzero(srt[0] - srt > lr.LOG_DBL_MIN)
                elif key == "khat_above":
                    assert ref["pareto_k"][col] > val, (w["name"], ref["pareto_k"][col])
                elif key == "khat_below":
                    assert ref["pareto_k"][col] < val, (w["name"], ref["pareto_k"][col])
                elif key == "constant":
                    assert ref["n_tail"][col] == 0 and ref["pareto_k"][col] == math.inf
                    assert ref["elpd_loo"][col] == val and ref["lppd"][col] == val and ref["p_waic"][col] == 0.0
                elif key == "bad":
                    assert ref["n_tail"][col] == 0
                    assert all(math.isnan(ref[f][col]) for f in ("elpd_loo", "pareto_k", "lppd", "p_waic"))
                else:
                    raise AssertionError(key)
    assert seen == {"n_tail", "no_fit", "m_min", "n_below_M", "khat_above", "khat_below", "constant", "bad", "floor"}


def test_poisoned_columns_leave_their_neighbours_alone():
    n = _by_name()
    bad, clean = lc.reference(n["poisoned"]), lc.reference(n["poisoned_clean_twin"])
    for col in (0, 1, 3, 6):
        for f in lr.FIELDS:
            assert bad[f][col] == clean[f][col]


def test_r_eff_and_window_worlds():
    n = _by_name()
    w = lc.worlds()[n["r_eff"]]
    assert w["r_eff"] is not None and not np.any(w["r_eff"] == 1.0)
    assert len(set(lc.reference(n["r_eff"])["n_tail"].tolist())) == 3
    w = lc.worlds()[n["window"]]
    g_from, g_to = w["window"]
    assert g_from > 1 and g_to < w["loglik"].shape[2] and (g_to - g_from + 1) % 2 == 1
