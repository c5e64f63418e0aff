"""Guard-band test of mdsp_resp_exec (INTEGRATION.md "What a call touches"; the layouts and checks of tests/guard_bands.py): w or the points and the output
sit inside larger allocations, 0 - 3 ELEMENTS off a 128-byte line -- input and output shifted alike and differently -- with a quiet-NaN poison around
the input and another NaN pattern all over the output buffer.  Per call: nothing outside [0, nw) of the output changed, every word inside written and
none NaN (a point read from outside the array is poison), and with POINTS input the result equals the host emulation bit for bit.  The coefficient
arrays are host arrays, copied when the plan is made: they sit in poisoned host buffers at odd offsets, which must come back unchanged -- a coefficient
read from outside them would be NaN in every output.  The device copies and the workspace of a cut belong to the plan and cannot be laid out by a
caller; what the launches do with them is covered by the bit equality of the result.  Every form, both types, the single launch and the forced cut."""
import numpy as np
import pytest

import guard_bands as gb
import response_cases as rc
import sos_cases as sc

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD
SHIFTS = ((0, 0), (1, 1), (2, 2), (3, 3), (3, 1), (0, 3))        # base_off of the input, of the output
NW = 131                                                         # three tiles of 64, the last one ragged


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _guarded_host(v, off):
    """v inside a poisoned host buffer, `off` elements behind its start: (the view handed to the library, the whole buffer)"""
    v = np.ascontiguousarray(v)
    real = np.float64
    flat = v.view(real).reshape(-1) if v.dtype.kind == "c" else v.astype(real).reshape(-1)
    buf = np.full(flat.size + 64, np.nan, dtype=real)
    buf[:] = np.frombuffer(np.uint64(gb.POISON[8]).tobytes() * buf.size, dtype=real)
    buf[17 + off:17 + off + flat.size] = flat
    return buf[17 + off:17 + off + flat.size], buf


def _cases(R):
    rng = np.random.default_rng(8)
    b = rng.standard_normal(53)
    a = np.concatenate([[1.0], 0.05 * rng.standard_normal(40)])
    tb, g = sc.table("butter5_02")
    z, p = 0.9 * np.exp(1j * rng.uniform(0, 6, 7)), 0.7 * np.exp(1j * rng.uniform(0, 6, 5))
    return (("poly", rc.POLY, b, a, 1.0, rc.DERIV), ("poly_fir", rc.POLY, b, None, 1.0, 0), ("sections", rc.SECTIONS, tb.reshape(-1), None, g, 0),
            ("zpk", rc.ZPK, z, p, 1.5, 0))


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("chunks", [0, 3], ids=["auto", "three_chunks"])
@pytest.mark.parametrize("case", range(4), ids=["poly", "poly_fir", "sections", "zpk"])
def test_resp_stays_inside_its_arrays(d, case, chunks, R):
    import ctypes as C
    import torch
    from dsp_jl_amd import _dev, _lib
    label, form, num, den, gain, flags = _cases(R)[case]
    ct = rc.ctype(R)
    pts = np.exp(1j * np.linspace(0.05, 6.2, NW)).astype(ct)
    w = np.linspace(0.05, 3.0, NW).astype(R)
    want = rc.emulate(form, R, num, den, pts, gain=gain, flags=flags, chunks=chunks)
    for k, (sx, sy) in enumerate(SHIFTS):
        what = f"resp {label} chunks {chunks} shift ({sx}, {sy})"
        nview, nbuf = _guarded_host(num, k % 4)
        dview, dbuf = (None, None) if den is None else _guarded_host(den, (k + 1) % 4)
        nkeep, dkeep = nbuf.copy(), None if dbuf is None else dbuf.copy()
        per = {rc.POLY: 1, rc.SECTIONS: 5, rc.ZPK: 2}[form]
        for in_mode, out_mode, arg, idt, odt in ((rc.POINTS, rc.COMPLEX, pts, ct, ct), (rc.W, rc.ANGLE, w, np.dtype(R), np.dtype(R))):
            h = C.c_void_p()
            _lib.check(_lib.lib().mdsp_resp_plan_create(C.byref(h), form, flags | (rc.NEG if form == rc.POLY else 0), out_mode, in_mode, _dev.md_dtype(R),
                                                        nview.ctypes.data_as(_lib.pdbl), nview.size // per,
                                                        None if dview is None else dview.ctypes.data_as(_lib.pdbl), 0 if dview is None else dview.size // per,
                                                        gain, 0.0, NW, chunks))
            try:
                info = [C.c_int64() for _ in range(3)]
                _lib.check(_lib.lib().mdsp_resp_plan_info(h, *[C.byref(v) for v in info]))
                assert info[0].value == (2 if form == rc.POLY and chunks == 3 else 1), what
                lx = gb.layout(NW, 1, NW, GUARD, GUARD, sx, idt)
                ly = gb.layout(NW, 1, NW, GUARD, GUARD, sy, odt)
                xd, yd = gb.to_device(gb.new_input(lx, arg.reshape(1, NW))), gb.to_device(gb.new_output(ly))
                _lib.check(_lib.lib().mdsp_resp_exec(h, gb.ptr(xd, lx), gb.ptr(yd, ly), _dev.stream_ptr()))
                after = gb.from_device(yd)
                gb.check_output(after, ly, NW, what)
                if in_mode == rc.POINTS:
                    assert np.array_equal(gb.columns(after, ly).view(np.uint8), np.ascontiguousarray(want.reshape(1, NW)).view(np.uint8)), what
                assert np.array_equal(gb.from_device(xd), gb.new_input(lx, arg.reshape(1, NW))), what + ": the input changed"
            finally:
                _lib.lib().mdsp_resp_plan_destroy(h)
        assert np.array_equal(nbuf.view(np.uint64), nkeep.view(np.uint64)), what + ": a host coefficient buffer changed"
        assert dbuf is None or np.array_equal(dbuf.view(np.uint64), dkeep.view(np.uint64)), what
    torch.cuda.synchronize()
