"""GPU: every generated dimension of window_kernel_pw and of the sixteen-lane regression kernel, bit for bit against the oracle.

Each dimension compiles DPP text of its own (demcz_pw_wdpp_<D>.inc, demcz_pw_ddpp_<D>.inc, demcz_ml_lrdpp_<D>.inc) and constants
of its own (demcz_kernels_pw.h: the DMA instructions per slot, the rounds of increment and history lanes, the counted wait built
from them, the row stride, the odd-D tail of the candidate row; demcz_kernels_ml.h: the resident design tiles).  lanes_per_chain
= 0 selects exactly these kernels for ordinary populations.  tests/dimension_cases.py holds the worlds: for pw one handle per
(target, d) whose schedule reaches all six forms -- REG / general LIVE, non-LIVE, each plain and tempered -- in which, by the
oracle alone (tests/test_dimension_cases.py), every accept / reject outcome of a pass occurs in every form; for the regression
target helper waves with resident, non-resident and partial rounds, and the kernel without helper waves.  No tolerance anywhere
(DESIGN.md section 3)."""
import os

import numpy as np
import pytest

import dimension_cases as dc
from helpers import SPLIT_WAVE

pytestmark = pytest.mark.gpu


def engine_run(demc, case, lanes, history=True):
    """The library over the case's pieces on one handle.  dimension_cases.oracle_run's dict (changed: the total), `names`: the
    kernel's name and the count of window launches after every piece, `layout` and `live_status`.  history = False: a handle that
    keeps none (Gcap = 0), chain and log_obj are None."""
    w, N, d, G = case["problem"], case["N"], case["d"], case["G"]
    M0 = w["Zinit"].shape[0]
    e = demc.HipEngine(N=N, d=d, K=case["K"], Mcap=M0 + N * (G // case["K"] + 1), Gcap=G if history else 0, blockindex=[range(d)],
                       eps_scale=w["eps_scale"], seed=case["seed"], target=w["target"], lanes_per_chain=lanes)
    try:
        layout = e.info()["lanes_per_chain"]
        e.set_state(w["Zinit"][-N:], None, w["Zinit"])
        names, launches = [], []
        for p in case["pieces"]:
            a, b, tempered = p[0], p[1], p[2]
            e.run(a, b, case["gamma"], case["temperature"][a - 1:b] if tempered else None)
            names.append(e.kernel_name())
            launches.append(e.info()["window_launches"])
        chain, lobj = e.get_history(1, G) if history else (None, None)
        X, lp, Z, M = e.get_state()
        return dict(chain=chain, log_obj=lobj, X=X, logp=lp, Z=np.array(Z[:M]), M=M, changed=e.changed_total(1, G), names=names,
                    launches=launches, layout=layout, live_status=tuple(e.live_status()))
    finally:
        e.close()


def _same_as_oracle(got, ref, what, keys=("chain", "log_obj", "X", "logp", "Z")):
    for k in keys:
        assert got[k].shape == ref[k].shape, f"{what}: {k}: shapes {got[k].shape}, oracle {ref[k].shape}"
        ne = got[k] != ref[k]
        assert np.array_equal(got[k], ref[k]), (f"{what}: {k} differs from the oracle in {int(ne.sum())} places, first at "
                                                f"{tuple(int(v[0]) for v in np.nonzero(ne))} (log_obj, chain: the last index is generation - 1)")
    assert got["M"] == ref["M"], what
    assert got["changed"] == int(ref["changed"].sum()), f"{what}: changed_total"


@pytest.mark.parametrize("d", dc.PW_DIMS)
@pytest.mark.parametrize("kind", ["mvn", "iso"])
def test_wave_per_chain_every_dimension_every_form(demc, oracle, kind, d):
    case = dc.pw_case(kind, d)
    got = engine_run(demc, case, 0)
    assert got["layout"] == SPLIT_WAVE
    for (a, b, _, form), name in zip(case["pieces"], got["names"]):
        assert name == dc.pw_kernel_name(kind, d, form), f"{kind} d = {d}, generations {a}..{b}: planned {form}, ran {name}"
    assert {p[3] for p in case["pieces"]} == set(dc.FORMS) and len(got["names"]) == len(case["pieces"])
    assert got["launches"] == list(range(1, len(case["pieces"]) + 1)), "a piece is one launch: the name read behind it is that launch's"
    assert got["live_status"] == (True, 0), "a LIVE launch timed out and was redone: the LIVE kernels did not produce these numbers"
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"{kind} d = {d}")


@pytest.mark.parametrize("coop", [True, False], ids=["coop", "nocoop"])
@pytest.mark.parametrize("d", dc.LR_DIMS)
def test_regression_every_dimension_sixteen_lanes(demc, oracle, d, coop):
    """Odd dimensions by the library's choice, even ones by name.  d = 10 with helper waves does not exist: those 1381
    observations fit LDS and run window_kernel_lr16 (dimension_cases.lr_kernel_name); its generated text runs in the other case."""
    case = dc.lr_case(d, coop)
    got = engine_run(demc, case, 0 if d % 2 else 16)
    assert got["layout"] == 16
    name = dc.lr_kernel_name(d, coop)
    for n in got["names"]:
        if coop and d != 10 and "flipped" in os.environ.get("DEMCZ_LIB", ""):      # (the -DML_LRDPP=0 build has no helper waves)
            assert n.startswith("demcz::window_kernel_ml<LINREG_SSE, %d, 16" % d), n
        else:
            assert n == name, f"d = {d}: {n}, expected {name}"
    _same_as_oracle(got, dc.oracle_run(oracle, case), f"regression d = {d}, {case['nobs']} observations")
