"""Every launch geometry of the arbitrary-rate kernel against the extended-precision reference (tests/arb_ref.py), through the C ABI.

For each row of tests/arb_cases.py: mdsp_arb_kernel_geometry (this device's compute units) reports the row's geometry for the main chunk -- so a
passing row is evidence about that path --, and a stream of nch channels (ldx > xlen) cut at {[37 + tp,] 1, an odd point near a third, tp - 2
samples more (every window in the history), the rest} gives, for every output of every channel,

    |y - ref| <= 2 (tp + 2) u absdot + 4 u_min          (per real component for complex signals)

with absdot = sum_k |pfb z| + alpha sum_k |dpfb z| over the output's window, u = 2^-24 when taps and signal are both single and 2^-53 otherwise,
u_min the smallest positive normal of that type (tests/test_arb_reference_cpu.py shows six subtly wrong kernels fail it).  The output buffers hold
outputlength + 1 samples per channel, start as NaN and have ldy > ycap: everything past nwritten stays NaN in every column, the body has none,
nwritten equals the reference's count; after every chunk (phi_accumulator, input_deficit) equal the reference's and the history is bit-identical.

Rows of one family (same types, filter, rate and state; different tile, MDSP_ARB_NCH, MDSP_ARB_PRIO, gy, channel count) are bit-identical to each
other channel by channel: every path performs the same fma chain in tap order and the same combination.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import arb_cases as ac
from arb_cases import CASES, case_id, geometry, reported
from arb_ref import accumulation_unit, arb_ref, excess

pytestmark = pytest.mark.gpu

IDS = [case_id(c) for c in CASES]
FAMILIES = {}
for _c in CASES:
    FAMILIES.setdefault(ac.family(_c), []).append(_c)
FAMILIES = {k: v for k, v in FAMILIES.items() if len(v) > 1}
MARGIN = {}                                                             # (taps, signal) -> largest |y - ref| / (u absdot) seen


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def compute_units():
    """From the query itself: one tile and 16384 channel groups give gy = 8 CUs."""
    from dsp_jl_amd import _lib
    out = (C.c_int64 * 8)()
    _lib.check(_lib.lib().mdsp_arb_kernel_geometry(1, 1, 1.0, _lib.F32, _lib.F32, 65535, 1, 0, out))
    assert out[3] > out[5] and out[5] % 8 == 0
    return int(out[5]) // 8


@functools.lru_cache(maxsize=None)
def run_row(c):
    """The row's stream through mdsp_firarb_exec with every check of the module docstring; returns the outputs of the whole stream (nch, total)."""
    import torch
    from dsp_jl_amd import _lib
    lib = _lib.lib()
    rate, nphi, hlen, td, xd, nch, knobs, state, _, expect = c
    lt = {"f32": _lib.F32, "f64": _lib.F64, "c32": _lib.C32, "c64": _lib.C64}
    cplx = xd[0] == "c"
    dbl = td == "f64" or xd in ("f64", "c64")
    ynp = (np.complex128 if dbl else np.complex64) if cplx else (np.float64 if dbl else np.float32)
    rdt = np.float64 if dbl else np.float32
    tp = -(-hlen // nphi)
    hl = tp - 1
    cu = compute_units()
    n, cuts, nouts = ac.plan(c, cu)
    assert nouts[-1] == max(nouts) and nouts[-1] % 16                  # the main chunk: a partial last tile and anchor block
    g = geometry(c, nouts[-1], 0)
    assert reported(g) == expect, f"geometry {dict(zip(('tile', 'span', 'nchg', 'groups', 'tiles', 'gy', 'taps_in_lds', 'lds_bytes'), g))}, the table says {expect}"
    if c[8] in (ac.LOOP1, ac.LOOP2):
        assert (g[3], g[5]) == (3, 1 if c[8] == ac.LOOP1 else 2)
    h = ac.taps(c)
    x = ac.signal(c, n)
    ldx = n + 7
    xpad = np.zeros((nch, ldx), dtype=x.dtype)
    xpad[:, :n] = x
    x_dev = torch.from_numpy(xpad).to("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    u, umin = accumulation_unit(h.dtype, x.dtype)
    acc, dfc, phi = ac.initial_state(c)
    hist = None
    pieces = []
    worst_ratio = 0.0
    nan = complex(float("nan"), float("nan")) if cplx else float("nan")
    fh = C.c_void_p()
    try:
        for k, v in knobs:
            _lib.set_tunable(k, v)
        _lib.check(lib.mdsp_firarb_create(C.byref(fh), h.ctypes.data_as(C.c_void_p), hlen, float(rate), nphi, lt[td], lt[xd], nch))
        if phi is not None:
            _lib.check(lib.mdsp_firarb_setphase(fh, C.c_double(phi)))
        for (a, b), nout in zip(zip(cuts[:-1], cuts[1:]), nouts):
            xlen = b - a
            ol = C.c_int64()
            _lib.check(lib.mdsp_firarb_outputlength(fh, xlen, C.byref(ol)))
            ycap = max(ol.value, 0) + 1                                # allocate_output, stream_filt.jl:639-655
            ldy = ycap + 5
            y = torch.full((nch, ldy), nan, dtype=getattr(torch, np.dtype(ynp).name), device="cuda")
            nw = C.c_int64(-1)
            _lib.check(lib.mdsp_firarb_exec(fh, x_dev[:, a:].data_ptr(), xlen, ldx, y.data_ptr(), ycap, ldy, C.byref(nw), stream))
            torch.cuda.synchronize()
            assert nw.value == nout, (a, b)
            yh = y.cpu().numpy()
            assert np.isnan(np.ascontiguousarray(yh[:, nout:]).view(rdt)).all(), (a, b)
            body = np.ascontiguousarray(yh[:, :nout])
            assert not np.isnan(body.view(rdt)).any(), (a, b)
            ref, ad, (acc, dfc, hist) = arb_ref(h, rate, nphi, x[:, a:b], acc, dfc, hist)
            worst, ratio = excess(body, ref, ad, tp, u, umin)
            worst_ratio = max(worst_ratio, ratio)
            if worst > 1.0:
                err = np.abs(body.astype(ref.dtype) - ref)
                ch, m = np.unravel_index(int(np.argmax(err)), err.shape)
                pytest.fail(f"chunk [{a}, {b}): {worst:.3g} x the bound; worst output channel {ch} index {m} of {nout} (tile {g[0]}): {body[ch, m]} vs {ref[ch, m]}")
            pa, al, pi, de, xi = C.c_double(), C.c_double(), C.c_int64(), C.c_int64(), C.c_int64()
            hd = np.empty((nch, max(hl, 1)), dtype=x.dtype)
            _lib.check(lib.mdsp_firarb_get_state(fh, C.byref(pa), C.byref(al), C.byref(pi), C.byref(de), C.byref(xi), hd.ctypes.data_as(C.c_void_p)))
            assert (pa.value, de.value) == (acc, dfc), (a, b)
            assert (al.value, pi.value) == (acc - np.floor(acc), 1 + int(np.floor(acc))), (a, b)
            if hl > 0:
                assert np.array_equal(hd.view(np.uint8), np.ascontiguousarray(hist).view(np.uint8)), (a, b)
            pieces.append(body)
    finally:
        if fh.value:
            _lib.check(lib.mdsp_firarb_destroy(fh))
        for k, v in knobs:
            _lib.set_tunable(k, None)
    MARGIN[(td, xd)] = max(MARGIN.get((td, xd), 0.0), worst_ratio)
    print(f"\nmargin {case_id(c)}: tp={tp} max|y-ref|/(u absdot)={worst_ratio:.3f} bound/(u absdot)={2 * (tp + 2)}")
    return np.concatenate(pieces, axis=1)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_arbitrary_rate_path_against_extended_precision_reference(d, c):
    run_row(c)


@pytest.mark.parametrize("fam", list(FAMILIES), ids=["r{}_p{}_h{}_{}_{}_{}".format(*f) for f in FAMILIES])
def test_geometries_of_a_family_are_bit_identical(d, fam):
    rows = FAMILIES[fam]
    ys = [run_row(c) for c in rows]
    assert len({reported(geometry(c, ac.plan(c, compute_units())[2][-1], 0)) + (c[5], c[6]) for c in rows}) > 1
    for c, y in zip(rows[1:], ys[1:]):
        k, m = min(y.shape[0], ys[0].shape[0]), min(y.shape[1], ys[0].shape[1])
        assert m > 0
        same = np.ascontiguousarray(y[:k, :m]).view(np.uint8) == np.ascontiguousarray(ys[0][:k, :m]).view(np.uint8)
        if not same.all():
            ch, byte = np.argwhere(~same)[0]
            pytest.fail(f"{case_id(c)} differs from {case_id(rows[0])}: first at channel {ch}, output {byte // y.dtype.itemsize}; "
                        f"{int((~same).sum())} bytes differ")


def test_measured_margins(d):
    """One MEASURED line per type pair (DESIGN 4.7 carries them): the largest |y - ref| / (u absdot) over all rows of the pair."""
    for c in CASES:
        run_row(c)
    pairs = sorted({(c[3], c[4]) for c in CASES})
    assert len(pairs) == 8
    for td, xd in pairs:
        tps = [-(-c[2] // c[1]) for c in CASES if (c[3], c[4]) == (td, xd)]
        print(f"\nMEASURED taps={td} x={xd}: max|y-ref|/(u absdot)={MARGIN[(td, xd)]:.3f} (bound/(u absdot) from {2 * (min(tps) + 2)} to {2 * (max(tps) + 2)})")
