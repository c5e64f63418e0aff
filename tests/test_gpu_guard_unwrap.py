"""Guard-band test of mdsp_unwrap_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py): the (inner, len, outer)
array sits inside a larger allocation, 0, 1 or 3 ELEMENTS off a 128-byte line -- input and output shifted alike and differently, so no 16-byte alignment
of either can be assumed -- with a quiet-NaN poison around the input and another NaN pattern all over the output buffer.  Per call: nothing outside
[0, inner len outer) of the output changed, every element inside written and none NaN (a sample read from outside the input -- the left neighbour of
sample 0 of the first line, which does not exist, or the tail of a 16-byte vector -- is poison and would turn the rest of a line into NaN), and the
result equals the serial recurrence.  Both routes, the cut forced to three segments (reduce, carries, apply) and the single pass, both element types."""
import numpy as np
import pytest

import guard_bands as gb
import unwrap_cases as uc
import unwrap_ref as ur

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD
SHIFTS = ((0, 0), (1, 1), (3, 3), (3, 1), (0, 3))        # base_off of the input, of the output


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("segments", [3, 1], ids=["three_segments", "single_pass"])
@pytest.mark.parametrize("shape", [(2, 1027, 1), (1, 65, 1), (3, 7, 1), (2, 301, 3), (1, 17, 65)], ids=lambda s: "x".join(map(str, s)))
def test_unwrap_stays_inside_its_arrays(d, shape, segments, dt):
    import torch
    from dsp_jl_amd import _lib
    outer, n, inner = shape
    case = uc.make("guard", uc.walk(outer * 1000 + n + inner, outer, n, inner, dt))
    ref = ur.unwrap_serial(case.m, 1)
    total = outer * n * inner
    plan = d.UnwrapPlan(inner, n, outer, dt, float(ur.default_range(dt)), segments)
    assert plan.segments == segments and plan.route == (_lib.UNWRAP_CONTIGUOUS if inner == 1 else _lib.UNWRAP_STRIDED)
    for sx, sy in SHIFTS:
        what = f"unwrap {shape} segments {segments} shift ({sx}, {sy})"
        lx = gb.layout(total, 1, total, GUARD, GUARD, sx, dt)
        ly = gb.layout(total, 1, total, GUARD, GUARD, sy, dt)
        xd, yd = gb.to_device(gb.new_input(lx, case.m.reshape(1, total))), gb.to_device(gb.new_output(ly))
        plan.exec(gb.ptr(xd, lx), gb.ptr(yd, ly))
        after = gb.from_device(yd)
        gb.check_output(after, ly, total, what)
        assert ur.equal(gb.columns(after, ly).reshape(shape), ref), what
        # in place: the input buffer is the output; its guards keep the poison
        before = gb.new_input(lx, case.m.reshape(1, total))
        xd = gb.to_device(before)
        plan.exec(gb.ptr(xd, lx), gb.ptr(xd, lx))
        got = gb.from_device(xd)
        body = slice(lx.col0, lx.col0 + total)
        outside = np.ones(lx.total, dtype=bool)
        outside[body] = False
        assert np.array_equal(got[outside], before[outside]), what + " in place: a guard word changed"
        assert ur.equal(got.view(dt)[body].reshape(shape), ref), what + " in place"
    torch.cuda.synchronize()
