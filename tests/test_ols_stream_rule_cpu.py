"""The footprint rule of the tiled overlap-save kernel's streaming cache policy (dsp.jl_amd/csrc/ols_plan.h ols_stream_rule) as pure host
arithmetic: mdsp_ols_stream_for reports whether a launch of a TILED plan over `columns` columns of nx samples / nout outputs runs the streaming
instantiation -- under the rule (MDSP_OLS_STREAM = 1) exactly when the bytes it reads plus the bytes it writes, (nx + nout) columns 4, exceed THRESHOLD.
Only real Float32 plans can be tiled, so no other dtype ever streams, and with MDSP_OLS_TILE = 0 no plan is tiled and nothing streams.  MDSP_OLS_STREAM
= 0 never streams, 2 streams every launch of a tiled plan (the tests' and the A/B's way to run the instantiation on small shapes).  No device."""
import ctypes as C

import pytest

from dsp_jl_amd import _lib

THRESHOLD = 512 << 20       # bytes; DESIGN.md 4.2: twice the Infinity Cache, from the measured sizes
DEFAULT = 1                 # MDSP_OLS_STREAM of the library as shipped: the rule
NB = 256


def stream_for(nx, nout, columns, dtype=_lib.F32):
    s = C.c_int(-1)
    _lib.check(_lib.lib().mdsp_ols_stream_for(nx, nout, columns, dtype, C.byref(s)))
    assert s.value in (0, 1)
    return s.value


class _knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        _lib.set_tunable(self.name, self.value)

    def __exit__(self, *exc):
        _lib.set_tunable(self.name, None)


def _edges(columns, conv):
    """(nx, nout) with the largest footprint at or below THRESHOLD and the smallest above it, for filt (nout = nx) and conv (nout = nx + nb - 1)."""
    extra = NB - 1 if conv else 0
    per = THRESHOLD // (4 * columns)              # samples read + written per column at the threshold (rounded down)
    nx = (per - extra) // 2
    below = (nx, nx + extra)
    assert (below[0] + below[1]) * columns * 4 <= THRESHOLD
    nx += 1
    while (2 * nx + extra) * columns * 4 <= THRESHOLD:
        nx += 1
    above = (nx, nx + extra)
    assert (2 * (nx - 1) + extra) * columns * 4 <= THRESHOLD < (above[0] + above[1]) * columns * 4
    return below, above


@pytest.mark.parametrize("columns", [1, 3])
@pytest.mark.parametrize("conv", [False, True], ids=["filt", "conv"])
def test_rule_switches_at_the_threshold(columns, conv):
    below, above = _edges(columns, conv)
    with _knob("MDSP_OLS_STREAM", 1):
        assert stream_for(*below, columns) == 0, below
        assert stream_for(*above, columns) == 1, above
        assert stream_for(1 << 30, 1 << 30, columns) == 1          # the headline shape
        assert stream_for(1 << 20, 1 << 20, columns) == 0
        assert stream_for(0, 0, columns) == 0


def test_default():
    below, above = _edges(1, False)
    assert stream_for(*below, 1) == 0
    assert stream_for(*above, 1) == (1 if DEFAULT == 1 else 0)


@pytest.mark.parametrize("dtype", [_lib.F64, _lib.C32, _lib.C64])
@pytest.mark.parametrize("knob", [0, 1, 2])
def test_untiled_dtypes_never_stream(dtype, knob):
    with _knob("MDSP_OLS_STREAM", knob):
        for columns in (1, 3):
            assert stream_for(1 << 30, 1 << 30, columns, dtype) == 0
            assert stream_for(1000, 1000, columns, dtype) == 0


@pytest.mark.parametrize("knob", [0, 1, 2])
def test_no_tiled_plans_no_streaming(knob):
    with _knob("MDSP_OLS_TILE", 0), _knob("MDSP_OLS_STREAM", knob):
        assert stream_for(1 << 30, 1 << 30, 1) == 0
        assert stream_for(1000, 1000, 3) == 0


def test_knob_overrides_the_rule():
    below, above = _edges(1, False)
    with _knob("MDSP_OLS_STREAM", 0):
        assert stream_for(*above, 1) == 0 and stream_for(1 << 30, 1 << 30, 3) == 0
    with _knob("MDSP_OLS_STREAM", 2):
        assert stream_for(*below, 1) == 1 and stream_for(1000, 1000, 1) == 1
    assert stream_for(*below, 1) == 0                               # the knob is back


def test_argument_errors():
    s = C.c_int(0)
    assert _lib.lib().mdsp_ols_stream_for(-1, 0, 1, _lib.F32, C.byref(s)) == _lib.ERR_ARGUMENT
    assert _lib.lib().mdsp_ols_stream_for(10, 10, 1, 99, C.byref(s)) == _lib.ERR_ARGUMENT
