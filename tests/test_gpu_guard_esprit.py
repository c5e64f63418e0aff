"""Guard-band tests of mdsp_hankel_gram_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py as they are): the signal
sits inside a larger allocation, 0 - 3 ELEMENTS off a 128-byte line, with a quiet-NaN poison all around it, and R goes into a buffer that holds another NaN
pattern everywhere, its M columns ldr = M + 3 apart: the padding rows of every column are guard.  A body tile, a halo or an edge that read one sample
outside the signal would carry a NaN into its sums and differ from the host emulation; every word of the result buffer outside R's columns must keep its
pattern, every word inside must be written.  The partials belong to the plan; what the body launch writes into them is covered by the bit equality of R."""
import numpy as np
import pytest

import esprit_cases as ec
import guard_bands as gb

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


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_hankel_gram_stays_inside_the_signal_and_the_matrix(d, dt):
    import torch
    dt = np.dtype(dt)
    T, G = ec.tile_and_group()
    odt = ec.out_dtype(dt)
    for n, M in ((1, 1), (3, 2), (G + 1 + T, G + 1), (3 * T + 5 + 2 * 5, 5)):
        x = ec.signal(n, dt, seed=n)
        ldr = M + 3
        for S in (1, 3):
            want = ec.emulate(x, M, S)
            plan = d.GramPlan(dt, n, M, S)
            for off in OFFSETS:
                what = f"hankel_gram {dt.name} n {n} M {M} segments {S} offset {off}"
                lx = gb.layout(n, 1, n, GUARD, GUARD, off, dt)
                lr = gb.layout(M, M, ldr, GUARD, GUARD, (off + 1) % 4, odt)
                before = gb.new_input(lx, x.reshape(1, n))
                xd, rd = gb.to_device(before), gb.to_device(gb.new_output(lr))
                plan.exec(gb.ptr(xd, lx), gb.ptr(rd, lr), ldr)
                after = gb.from_device(rd)
                gb.check_output(after, lr, M, what)
                assert gb.columns(after, lr).T.tobytes() == want.tobytes(), what
                assert np.array_equal(gb.from_device(xd), before), what + ": the signal's buffer changed"
    torch.cuda.synchronize()
