"""Program targets on the wave-per-chain layout (DEMCZ_LAYOUT_PROGRAM_WAVE), CPU tier: the unit hipRTC compiles for such a handle
(window_kernel_ps for d = 2..5, window_kernel_pw for d = 6..32, with the user's demcz_logobj called once per node lane) needs no
device to compile, so demcz_program_check_layout and ProgramTarget.check(layout=) are exercised here.  The runs on the device are
in test_gpu_program_wave.py."""
import ctypes as C
import re
import time
from pathlib import Path

import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib
from program_texts import LINREG, LOGISTIC, ROSENBROCK, SYNTAX_ERROR

ROOT = Path(__file__).resolve().parent.parent
WAVE = _lib.LAYOUT_PROGRAM_WAVE


def _check(d, src, layout, options=None):
    L = _lib.load()
    rc = L.demcz_program_check_layout(d, src.encode(), None if options is None else options.encode(), layout)
    return rc, (L.demcz_last_error(None) or b"").decode()


def test_constant_is_the_headers_and_free():
    hdr = (ROOT / "include" / "demcz.h").read_text()
    vals = {n: int(v) for n, v in re.findall(r"#define (DEMCZ_LAYOUT_\w+) (\d+)", hdr)}
    assert vals["DEMCZ_LAYOUT_PROGRAM_WAVE"] == WAVE == demc.LAYOUT_PROGRAM_WAVE
    assert len(set(vals.values())) == len(vals) and WAVE not in (0, 1, 8, 16)
    jl = (ROOT / "julia" / "DEMCHip.jl").read_text()
    assert re.search(rf"const LAYOUT_PROGRAM_WAVE = Int32\({WAVE}\)", jl)


@pytest.mark.parametrize("d", [2, 5, 6, 7, 20, 32])
def test_rosenbrock_compiles_for_the_wave_layout(d):
    """d = 2, 5: window_kernel_ps; 6, 7, 20, 32: window_kernel_pw."""
    rc, msg = _check(d, ROSENBROCK, WAVE)
    assert rc == _lib.OK, msg


def test_programs_with_data_loads_local_arrays_and_transcendentals_compile():
    for d, src in ((6, LINREG), (4, LOGISTIC), (9, LOGISTIC)):
        rc, msg = _check(d, src, WAVE)
        assert rc == _lib.OK, msg


@pytest.mark.parametrize("d", [1, 33])
def test_dimension_out_of_range_is_refused_with_a_message(d):
    rc, msg = _check(d, ROSENBROCK, WAVE)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert ("needs d in 2..32" if d == 1 else "d must be in 1..32") in msg, msg


def test_unknown_layout_is_refused():
    for layout in (8, 16, _lib.LAYOUT_SPLIT, _lib.LAYOUT_SPLIT_WAVE):
        rc, msg = _check(5, ROSENBROCK, layout)
        assert rc == _lib.ERR_INVALID_ARGUMENT and "lanes_per_chain must be 0 or 1" in msg


def test_syntax_error_names_identifier_and_the_users_line():
    rc, msg = _check(7, SYNTAX_ERROR, WAVE)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "undefined_thing" in msg
    assert "program:4:" in msg            # the user's own line number, file "program"
    rc, msg = _check(3, SYNTAX_ERROR, WAVE)
    assert rc == _lib.ERR_INVALID_ARGUMENT and "program:4:" in msg


def test_two_units_two_cache_entries():
    """The one-lane unit and the wave unit of one program are different compilations; each is cached on its own.  (A unique
    program text: nothing else in this process has compiled it.)  A cached call returns in well under a tenth of a compile --
    DESIGN.md section 4.12: 0.28 s against 0.3 ms for the one-lane unit."""
    src = ROSENBROCK.replace("return -s;", "return -(s + 0.0 * 20261016.0);")

    def timed(layout):
        t0 = time.perf_counter()
        rc, msg = _check(5, src, layout)
        assert rc == _lib.OK, msg
        return time.perf_counter() - t0

    lane_first = timed(1)
    wave_first = timed(WAVE)            # not a hit of the one-lane entry: it compiles
    wave_second = timed(WAVE)
    lane_second = timed(0)              # 0 and 1 are the same unit
    print(f"one-lane unit {lane_first:.3f} s then {lane_second * 1e3:.2f} ms; wave unit {wave_first:.3f} s then {wave_second * 1e3:.2f} ms")
    assert wave_second <= wave_first / 10
    assert lane_second <= lane_first / 10
    assert wave_first >= 10 * lane_second          # the wave check after the one-lane check was a compile, not a cache hit


def test_program_target_check_takes_a_layout():
    demc.ProgramTarget(ROSENBROCK, 7).check(layout=WAVE)
    demc.ProgramTarget(ROSENBROCK, 7).check(layout=0)
    with pytest.raises(demc.DemczError) as ei:
        demc.ProgramTarget(SYNTAX_ERROR, 7).check(layout=WAVE)
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT and "undefined_thing" in str(ei.value) and "program:4:" in str(ei.value)
    with pytest.raises(demc.DemczError):
        demc.ProgramTarget(ROSENBROCK, 1).check(layout=WAVE)


def test_symbol_is_exported_and_listed():
    lib = C.CDLL(str(demc.LIB_PATH))
    assert "demcz_program_check_layout" in demc.SYMBOLS
    getattr(lib, "demcz_program_check_layout")
