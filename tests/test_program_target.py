"""Program targets (DEMCZ_TARGET_PROGRAM), CPU tier: compiling a user's log-density with hipRTC for gfx950 needs no device, so
demcz_program_check and ProgramTarget.check() are exercised here.  The runs on the device are in test_gpu_program_target.py."""
import ctypes as C

import pytest

import demc_jl_amd as demc
from demc_jl_amd import _lib

ROSENBROCK = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double s = 0.0;
    for (int i = 0; i + 1 < DEMCZ_D; ++i) {
        const double a = x[i + 1] - x[i] * x[i];
        const double b = 1.0 - x[i];
        s = s + 100.0 * (a * a) + b * b;
    }
    return -s;
}
"""

# logistic regression: data = design (NOBS x DEMCZ_D, row-major) || labels (NOBS)
LOGISTIC = """
__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    const int64_t nobs = ndata / (DEMCZ_D + 1);
    const double* y = data + nobs * DEMCZ_D;
    double s = 0.0;
    for (int64_t o = 0; o < nobs; ++o) {
        double eta = 0.0;
        for (int j = 0; j < DEMCZ_D; ++j) eta = eta + data[o * DEMCZ_D + j] * x[j];
        s = s + y[o] * eta - log1p(exp(eta));
    }
    return s;
}
"""

SYNTAX_ERROR = """__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)
{
    double s = x[0];
    s = s + undefined_thing;
    return -s;
}
"""


def _check(d, src, options=None):
    L = _lib.load()
    rc = L.demcz_program_check(d, src.encode(), None if options is None else options.encode())
    return rc, (L.demcz_last_error(None) or b"").decode()


@pytest.mark.parametrize("d", [1, 7, 32])
def test_rosenbrock_compiles(d):
    rc, msg = _check(d, ROSENBROCK)
    assert rc == _lib.OK, msg


def test_program_with_data_and_transcendentals_compiles():
    rc, msg = _check(4, LOGISTIC, "-DUNUSED_SWITCH=1")
    assert rc == _lib.OK, msg


def test_syntax_error_names_identifier_and_line():
    rc, msg = _check(7, SYNTAX_ERROR)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "undefined_thing" in msg
    assert "program:4:" in msg            # the user's own line number


def test_missing_logobj_is_rejected_with_a_message():
    rc, msg = _check(3, "__device__ double f(const double* x) { return x[0]; }\n")
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "does not define demcz_logobj" in msg


@pytest.mark.parametrize("d", [0, 33])
def test_dimension_out_of_range_is_rejected(d):
    rc, msg = _check(d, ROSENBROCK)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "1..32" in msg


def test_user_options_reach_the_compiler():
    src = "#ifndef NEEDED\n#error NEEDED is not defined\n#endif\n" + ROSENBROCK
    rc, msg = _check(5, src)
    assert rc == _lib.ERR_INVALID_ARGUMENT and "NEEDED is not defined" in msg
    rc, msg = _check(5, src, "-DNEEDED=1")
    assert rc == _lib.OK, msg


def test_program_target_check_raises_with_the_log():
    with pytest.raises(demc.DemczError) as ei:
        demc.ProgramTarget(SYNTAX_ERROR, 7).check()
    assert ei.value.code == _lib.ERR_INVALID_ARGUMENT
    assert "undefined_thing" in str(ei.value) and "program:4:" in str(ei.value)
    demc.ProgramTarget(ROSENBROCK, 7, options=["-DUNUSED=1"]).check()


def test_program_target_is_exported_device_target():
    t = demc.ProgramTarget(ROSENBROCK, 3, data=[1.0, 2.0])
    assert demc.is_device_target(t)
    assert t.kind == _lib.TARGET_PROGRAM == 4
    assert "ProgramTarget" in dir(demc)


def test_program_symbols_are_exported():
    lib = C.CDLL(str(demc.LIB_PATH))
    for name in ("demcz_program_check", "demcz_set_program"):
        assert name in demc.SYMBOLS
        getattr(lib, name)
