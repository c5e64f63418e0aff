"""Guard-band test of mdsp_sos_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py): the columns sit inside a
larger allocation, 0, 1 or 3 ELEMENTS off a 128-byte line -- input and output shifted alike and differently -- with padding between the columns, a
quiet-NaN poison around the input and another NaN pattern all over the output buffer; the state array sits in a guarded allocation of its own.  Per call:
nothing outside [0, n) of each output column changed, every element inside written and none NaN (a sample read from outside a column is poison and never
leaves the line again), the state's guards untouched, and the result equals the host emulation bit for bit.  The cut forced to three segments (end states,
carries, apply) and the single pass, both real types and ComplexF32, out of place and in place.  The workspace of a cut belongs to the plan and cannot be
laid out by a caller; what the three launches write into it is covered by the bit equality of the result."""
import numpy as np
import pytest

import guard_bands as gb
import sos_cases as sc

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD
SHIFTS = ((0, 0), (1, 1), (3, 3), (3, 1), (0, 3))        # base_off of the input, of the output
TILE = 1024


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("segments", [3, 1], ids=["three_segments", "single_pass"])
@pytest.mark.parametrize("shape", [(1, 65), (3, 7), (2, TILE + 3)], ids=lambda s: "x".join(map(str, s)))
def test_sos_stays_inside_its_arrays(d, shape, segments, dt):
    import torch
    ncols, n = shape
    tb, g = sc.table("butter5_02")
    K = len(tb)
    assert d.sos_geometry(K, dt, n, ncols, segments)[2] == TILE
    plan = d.SosPlan(tb, g, dt, n, ncols, segments)
    assert plan.segments == segments
    ld = n + 5
    x = sc.signal(n, ncols, dt, salt=n).reshape(n, ncols)
    st0 = (0.1 * sc.signal(2 * K, ncols, dt, salt=n + 1)).reshape(2, K, ncols)
    want, st_want = sc.emulate(tb, g, x, dt, segments, state=st0)
    want = want.T
    st_cols = np.ascontiguousarray(st0.transpose(2, 1, 0)).reshape(1, ncols * 2 * K)
    ls = gb.layout(ncols * 2 * K, 1, ncols * 2 * K, GUARD, GUARD, 1, dt)
    body_s = slice(ls.col0, ls.col0 + ncols * 2 * K)
    for sx, sy in SHIFTS:
        what = f"sos {shape} segments {segments} shift ({sx}, {sy})"
        lx = gb.layout(n, ncols, ld, GUARD, GUARD, sx, dt)
        ly = gb.layout(n, ncols, ld, GUARD, GUARD, sy, dt)
        s_before = gb.new_input(ls, st_cols)
        xd, yd, sd = gb.to_device(gb.new_input(lx, x.T)), gb.to_device(gb.new_output(ly)), gb.to_device(s_before)
        plan.exec(gb.ptr(xd, lx), ld, gb.ptr(yd, ly), ld, gb.ptr(sd, ls))
        after = gb.from_device(yd)
        gb.check_output(after, ly, n, what)
        assert np.array_equal(gb.columns(after, ly).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what
        s_after = gb.from_device(sd)
        k, _ = gb.words(ls)
        outside = np.ones(ls.total * k, dtype=bool)
        outside[body_s.start * k:body_s.stop * k] = False
        assert np.array_equal(s_after[outside], s_before[outside]), what + ": a guard word of the state changed"
        got_state = s_after.view(dt)[body_s].reshape(ncols, K, 2).transpose(2, 1, 0)
        assert np.array_equal(np.ascontiguousarray(got_state).view(np.uint8), np.ascontiguousarray(st_want).view(np.uint8)), what + " (end state)"
        # in place: the input buffer is the output; its guards and the padding between the columns keep the poison
        before = gb.new_input(lx, x.T)
        xd, sd = gb.to_device(before), gb.to_device(s_before)
        plan.exec(gb.ptr(xd, lx), ld, gb.ptr(xd, lx), ld, gb.ptr(sd, ls))
        got = gb.from_device(xd)
        kx, _ = gb.words(lx)
        outside = np.ones(lx.total * kx, dtype=bool)
        for c in range(ncols):
            outside[lx.starts[c] * kx:(lx.starts[c] + n) * kx] = False
        assert np.array_equal(got[outside], before[outside]), what + " in place: a guard word changed"
        assert np.array_equal(gb.columns(got, lx).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what + " in place"
    torch.cuda.synchronize()
