"""Guard-band tests of mdsp_reduce_exec and mdsp_shift_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py): the
array sits inside a larger allocation, 0 - 3 ELEMENTS off a 128-byte line, with a quiet-NaN poison all around it, and the result goes into a buffer that
holds another NaN pattern everywhere.  A reduction that read one element outside its lines would sum a NaN (or raise the NaN flag of ABSARGMAX) and differ
from the host emulation; every word of the result buffer outside the results must keep its pattern, every word inside must be written.  A shift must leave
every word outside the line as it was -- in place the input buffer's poison, out of place the output buffer's fill -- and the line must equal numpy's."""
import numpy as np
import pytest

import guard_bands as gb
import util_cases as uc
import util_ref as ur

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.mark.parametrize("op_dt", uc.OPS, ids=uc.op_id)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 65, 1), (1, 257, 1), (3, 1023, 1), (1, 63, 2), (2, 257, 3), (1, 64, 65)], ids=lambda s: "x".join(map(str, s)))
def test_reductions_stay_inside_their_arrays(d, shape, op_dt):
    import torch
    from dsp_jl_amd import _lib
    op, dt = op_dt
    outer, n, inner = shape
    total, lines, words = outer * n * inner, outer * inner, uc.OUT_WORDS[op]
    centre = n // 2
    x = uc.reduce_input(op, dt, 17 + n, outer, n, inner, centre, (1, n // 2, n - 1))
    for seg in (0, 1, 3):
        plan = d.ReducePlan(inner, n, outer, op, dt, step=uc.STEP, centre=centre, segments=seg)
        for off in uc.OFFSETS:
            what = f"{uc.op_id(op_dt)} {shape} segments {seg} offset {off}"
            lx = gb.layout(total, 1, total, GUARD, GUARD, off, dt)
            ly = gb.layout(lines * words, 1, lines * words, GUARD, GUARD, off % 2, np.float64)
            xd, yd = gb.to_device(gb.new_input(lx, x.reshape(1, total))), gb.to_device(gb.new_output(ly))
            plan.exec(gb.ptr(xd, lx), gb.ptr(yd, ly))
            after = gb.from_device(yd)
            gb.check_output(after, ly, lines * words, what)
            got = gb.columns(after, ly).reshape(-1).view(np.int64)
            phase = off % (16 // dt.itemsize) if inner == 1 else 0
            want = np.ascontiguousarray(uc.emulate(x, op, uc.STEP, centre, seg, phase)[0]).reshape(-1).view(np.int64)
            assert np.array_equal(got, want), what
    torch.cuda.synchronize()


@pytest.mark.parametrize("esize", [4, 8, 16])
@pytest.mark.parametrize("tile", [64])
def test_shifts_stay_inside_their_line(d, tile, esize):
    import torch
    dt = np.dtype(uc.SHIFT_DTYPES[esize])
    for l in (1, 3, tile - 1, tile + 1, 2 * tile + 1, 5 * tile + 3):
        x = uc.gaussian(l, (l,), dt)
        for s in sorted({0, 1, -1, 15, -17, tile, -tile, l // 2, -(l // 2) - 1, l - 1, -l, l}):
            if abs(s) > l:
                continue
            want = ur.shiftsignal(x, s)
            for route in uc.ROUTES:
                for sx, sy in ((0, 0), (1, 3), (3, 1), (2, 2)):
                    what = f"shift {dt.name} l {l} s {s} route {uc.ROUTE_NAME[route]} offsets ({sx}, {sy})"
                    lx = gb.layout(l, 1, l, GUARD, GUARD, sx, dt)
                    before = gb.new_input(lx, x.reshape(1, l))
                    if uc.route_allowed(l, s, False, route):
                        ly = gb.layout(l, 1, l, GUARD, GUARD, sy, dt)
                        xd, yd = gb.to_device(before), gb.to_device(gb.new_output(ly))
                        d.ShiftPlan(l, s, esize, False, tile, route).exec(gb.ptr(xd, lx), gb.ptr(yd, ly))
                        after = gb.from_device(yd)
                        gb.check_output(after, ly, l, what)
                        assert np.array_equal(gb.columns(after, ly)[0], want) and np.array_equal(gb.from_device(xd), before), what
                    if uc.route_allowed(l, s, True, route):
                        xd = gb.to_device(before)
                        d.ShiftPlan(l, s, esize, True, tile, route).exec(gb.ptr(xd, lx), gb.ptr(xd, lx))
                        got = gb.from_device(xd)
                        expect = before.copy()
                        expect.view(dt)[lx.col0:lx.col0 + l] = want
                        assert np.array_equal(got, expect), what + " in place"
    torch.cuda.synchronize()
