"""Guard-band tests of mdsp_burg_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py as they are): the signal sits
inside a larger allocation, 0 - 3 ELEMENTS off a 128-byte line, with a quiet-NaN poison all around it, and the record goes into a buffer that holds another
NaN pattern everywhere.  A sweep or a finish that read one sample outside the signal would carry a NaN into its sums and differ from the host emulation;
every word of the result buffer outside the record must keep its pattern, every word inside must be written.  The work arrays belong to the plan; what the
launches write into them is covered by the bit equality of the record."""
import numpy as np
import pytest

import guard_bands as gb
import lpc_cases as lc

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD
OFFSETS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_burg_stays_inside_the_signal_and_the_record(d, dt):
    import torch
    dt = np.dtype(dt)
    tile = lc.tile_of(dt)
    for n, p in ((2, 1), (tile + 1, 3), (2 * tile + 3, 3), (2 * tile + 3, 0)):
        x = lc.signal("ar3", n, dt, seed=n)
        nrec = 2 * p + 2
        for S in (1, 3):
            want = lc.emulate_record(x, p, S)
            plan = d.BurgPlan(dt, n, S)
            for off in OFFSETS:
                what = f"burg {dt.name} n {n} p {p} segments {S} offset {off}"
                lx = gb.layout(n, 1, n, GUARD, GUARD, off, dt)
                ly = gb.layout(nrec, 1, nrec, GUARD, GUARD, (off + 1) % 4, dt)
                before = gb.new_input(lx, x.reshape(1, n))
                xd, yd = gb.to_device(before), gb.to_device(gb.new_output(ly))
                plan.exec(gb.ptr(xd, lx), p, gb.ptr(yd, ly))
                after = gb.from_device(yd)
                gb.check_output(after, ly, nrec, what)
                assert gb.columns(after, ly).reshape(-1).tobytes() == want.tobytes(), what
                assert np.array_equal(gb.from_device(xd), before), what + ": the signal's buffer changed"
    torch.cuda.synchronize()
