"""Predictive programs (demcz_predict, demcz_ppc), CPU tier: compiling a program with hipRTC for gfx950 needs no device, so
demcz_predict_check and PredictiveProgram.check() are exercised here.  The runs on the device are in test_gpu_predict.py."""
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib

import predict_cases as pc

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("demcz_predict_check", "demcz_predict", "demcz_predict_array", "demcz_ppc", "demcz_ppc_array")


def _check(d, m, src, options=None):
    L = _lib.load()
    rc = L.demcz_predict_check(d, m, src.encode(), None if options is None else options.encode())
    return rc, (L.demcz_last_error(None) or b"").decode()


@pytest.mark.parametrize("case", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_every_case_compiles(case):
    name, text, d, m, _ = case
    demc.PredictiveProgram(text, d, m).check()


def test_syntax_error_carries_the_users_line_number():
    with pytest.raises(demc.DemczError) as ei:
        demc.PredictiveProgram(pc.SYNTAX_ERROR, 3, 2).check()
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT
    assert "undefined_thing" in str(ei.value) and "program:4:" in str(ei.value)
    assert "predictive program" in str(ei.value) and "does not define demcz_predict" not in str(ei.value)


def test_source_without_demcz_predict_gets_the_hint():
    with pytest.raises(demc.DemczError) as ei:
        demc.PredictiveProgram(pc.NO_ENTRY_POINT, 3, 2).check()
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT
    assert "does not define demcz_predict" in str(ei.value) and "demcz_rng* rng, double* out" in str(ei.value)


@pytest.mark.parametrize("d,m", [(3, 0), (3, 33), (33, 2), (0, 2)])
def test_limits_are_invalid_argument_and_named(d, m):
    rc, msg = _check(d, m, pc.GENERIC)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "1..32" in msg and ("m must" in msg if 1 <= d <= 32 else "d must" in msg)


def test_null_source_is_invalid_argument():
    assert _lib.load().demcz_predict_check(3, 2, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_user_options_reach_the_compiler():
    src = "#ifndef NEEDED\n#error NEEDED is not defined\n#endif\n" + pc.GENERIC
    rc, msg = _check(5, 2, src)
    assert rc == _lib.ERR_INVALID_ARGUMENT and "NEEDED is not defined" in msg
    demc.PredictiveProgram(src, 5, 2, options=["-DNEEDED=1"]).check()


def test_second_check_of_a_program_is_a_cache_hit(tmp_path):
    """With DEMCZ_PROGRAM_DUMP set every COMPILATION writes its code object into that directory; a program taken from the
    process-wide cache writes nothing.  The key holds m: the same text with another m is another compilation."""
    src = "// predict cache probe\n" + pc.ONE_UNIFORM
    old = os.environ.get("DEMCZ_PROGRAM_DUMP")
    os.environ["DEMCZ_PROGRAM_DUMP"] = str(tmp_path)
    try:
        demc.PredictiveProgram(src, 2, 1).check()
        first = sorted(p.name for p in tmp_path.iterdir())
        assert len(first) == 1 and first[0].startswith("demcz_program_predict_d2_")
        demc.PredictiveProgram(src, 2, 1).check()
        assert len(list(tmp_path.iterdir())) == 1, "the second check compiled again"
        demc.PredictiveProgram(src, 2, 2).check()
        assert len(list(tmp_path.iterdir())) == 2, "m is part of the key"
    finally:
        if old is None:
            del os.environ["DEMCZ_PROGRAM_DUMP"]
        else:
            os.environ["DEMCZ_PROGRAM_DUMP"] = old


def test_program_d_must_be_the_arrays():
    """A host-side refusal: raised before the library is asked for anything."""
    prog = demc.PredictiveProgram(pc.GENERIC, 3, 2)
    chain = np.zeros((4, 5, 2), order="F")
    with pytest.raises(ValueError):
        demc.predict_chain(chain, None, prog, seed=1)
    with pytest.raises(ValueError):
        demc.ppc_chain(chain, None, prog, seed=1)
    with pytest.raises(ValueError):
        demc.ppc_chain(np.zeros((4, 3, 2), order="F"), None, prog, seed=1, observed=[0.0])         # (m = 2 values are needed)


def test_names_must_have_m_entries():
    assert demc.PredictiveProgram(pc.GENERIC, 3, 2, names=["a", "b"]).names == ["a", "b"]
    with pytest.raises(ValueError):
        demc.PredictiveProgram(pc.GENERIC, 3, 2, names=["a"])


def test_ppc_record():
    r = demc.ppc_record([3, 1, 0, 0, 4, 2], 10, ["a", "b"])
    assert r.gt.tolist() == [3, 0] and r.eq.tolist() == [1, 4] and r.nan.tolist() == [0, 2] and r.total == 10 and r.names == ["a", "b"]
    assert r.p_value.tolist() == [0.4, 0.5] and r.mid_p.tolist() == [0.35, 0.25]
    s = r + r
    assert s.total == 20 and s.gt.tolist() == [6, 0] and s.p_value.tolist() == r.p_value.tolist()


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(str(demc.LIB_PATH))
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "demcz.h").read_text(), flags=re.S)
    jl = (ROOT / "julia" / "DEMCHip.jl").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in demc.SYMBOLS and hasattr(lib, name), name
        assert f"(:{name}, libdemcz)" in jl, name
    for name in ("PredictiveProgram", "PPC", "predict_chain", "ppc_chain"):
        assert name in dir(demc)
    assert hasattr(demc.HipEngine, "predict") and hasattr(demc.DerivedHistory, "ppc")
