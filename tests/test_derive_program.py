"""Derive programs (demcz_derive), CPU tier: compiling a program with hipRTC for gfx950 needs no device, so demcz_derive_check and
DerivedProgram.check() are exercised here, and the NumPy restatements of tests/derive_cases.py are checked against a plain
per-draw loop.  The runs on the device are in test_gpu_derive.py."""
import ctypes as C
import os

import numpy as np
import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib

import derive_cases as dc


def _check(d, m, src, options=None):
    L = _lib.load()
    rc = L.demcz_derive_check(d, m, src.encode(), None if options is None else options.encode())
    return rc, (L.demcz_last_error(None) or b"").decode()


@pytest.mark.parametrize("case", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_every_case_compiles(case):
    name, text, d, m, data, _, _, _ = case
    demc.DerivedProgram(text, d, m, data=data).check()


def test_syntax_error_carries_the_users_line_number():
    with pytest.raises(demc.DemczError) as ei:
        demc.DerivedProgram(dc.SYNTAX_ERROR, 3, 2).check()
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT
    assert "undefined_thing" in str(ei.value) and "program:4:" in str(ei.value)
    assert "does not define demcz_derive" not in str(ei.value)        # (the hint is for a source without the entry point)


def test_source_without_demcz_derive_gets_the_hint():
    with pytest.raises(demc.DemczError) as ei:
        demc.DerivedProgram(dc.NO_ENTRY_POINT, 3, 2).check()
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT
    assert "does not define demcz_derive" in str(ei.value)
    assert "const double* x, double logp, const double* data, int64_t ndata, double* out" in str(ei.value)


@pytest.mark.parametrize("d,m", [(3, 0), (3, 33), (33, 2), (0, 2)])
def test_limits_are_invalid_argument_and_named(d, m):
    rc, msg = _check(d, m, dc.GENERIC)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "1..32" in msg and ("m must" in msg if 1 <= d <= 32 else "d must" in msg)


def test_null_source_is_invalid_argument():
    L = _lib.load()
    assert L.demcz_derive_check(3, 2, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_user_options_reach_the_compiler():
    src = "#ifndef NEEDED\n#error NEEDED is not defined\n#endif\n" + dc.GENERIC
    rc, msg = _check(5, 2, src)
    assert rc == _lib.ERR_INVALID_ARGUMENT and "NEEDED is not defined" in msg
    demc.DerivedProgram(src, 5, 2, options=["-DNEEDED=1"]).check()


def test_second_check_of_a_program_is_a_cache_hit(tmp_path):
    """With DEMCZ_PROGRAM_DUMP set every COMPILATION writes its code object into that directory; a program taken from the
    process-wide cache writes nothing.  The key holds m: the same text with another m is another compilation."""
    src = "// cache probe\n" + dc.GENERIC
    old = os.environ.get("DEMCZ_PROGRAM_DUMP")
    os.environ["DEMCZ_PROGRAM_DUMP"] = str(tmp_path)
    try:
        demc.DerivedProgram(src, 6, 2).check()
        first = sorted(p.name for p in tmp_path.iterdir())
        assert len(first) == 1 and first[0].startswith("demcz_program_derive_d6_")
        (tmp_path / first[0]).unlink()
        demc.DerivedProgram(src, 6, 2).check()
        assert list(tmp_path.iterdir()) == [], "the second check compiled again"
        demc.DerivedProgram(src, 6, 3).check()
        assert len(list(tmp_path.iterdir())) == 1, "m is part of the key"
    finally:
        if old is None:
            del os.environ["DEMCZ_PROGRAM_DUMP"]
        else:
            os.environ["DEMCZ_PROGRAM_DUMP"] = old


def test_a_derive_unit_and_a_target_unit_do_not_share_a_key():
    """One text that defines both entry points: checked as a derive program and as a program target, each compiles its own unit."""
    both = dc.SECOND + "\n__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata) { return -x[0] * x[0]; }\n"
    demc.DerivedProgram(both, 3, 2).check()
    demc.ProgramTarget(both, 3).check()
    demc.DerivedProgram(both, 3, 2).check()


@pytest.mark.parametrize("case", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_restatement_agrees_with_a_per_draw_loop(case):
    name, _, d, m, data, f, draw, exact = case
    N, G = 3, 4
    chain, log_obj = dc.history(N, d, G, seed=11)
    chain[0, 0, 0], chain[1, 0, 1] = -0.0, -1.25
    got = f(chain, log_obj) if data is None else f(chain, log_obj, data)
    assert got.shape == (N, m, G) and got.flags.f_contiguous
    for c in range(N):
        for g in range(G):
            x = [float(v) for v in chain[c, :, g]]
            want = draw(x, float(log_obj[c, g])) if data is None else draw(x, float(log_obj[c, g]), data)
            for k in range(m):
                a, b = float(got[c, k, g]), float(want[k])
                if exact:
                    assert (a != a and b != b) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (name, c, k, g, a, b)
                else:
                    assert abs(a - b) <= dc.REL_TOL * abs(b), (name, c, k, g, a, b)


def test_restatement_without_log_obj_sees_nan():
    f = dc.generic_numpy(3)
    chain, _ = dc.history(2, 2, 2, seed=3)
    out = f(chain, None)
    assert np.isnan(out[:, 2, :]).all() and not np.isnan(out[:, :2, :]).any()


def test_launch_constants_are_readable_from_the_kernel_header():
    threads, max_wg = _lib.derive_launch_constants()
    assert threads % 64 == 0 and threads >= 64 and max_wg >= 1


def test_names_must_have_m_entries():
    assert demc.DerivedProgram(dc.GENERIC, 3, 2, names=["a", "b"]).names == ["a", "b"]
    with pytest.raises(ValueError):
        demc.DerivedProgram(dc.GENERIC, 3, 2, names=["a"])


def test_symbols_are_exported():
    lib = C.CDLL(str(demc.LIB_PATH))
    for name in ("demcz_derive_check", "demcz_derive", "demcz_derive_array"):
        assert name in demc.SYMBOLS
        getattr(lib, name)
    for name in ("DerivedProgram", "DerivedHistory", "derive_chain"):
        assert name in dir(demc)
