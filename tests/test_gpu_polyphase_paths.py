"""Every polyphase FIR kernel path against the extended-precision reference (tests/polyphase_ref.py), through the C ABI.

For each row of tests/fir_cases.py: the filter reports the row's kernel path (so no comparison here is a kernel against itself), every
mdsp_fir_exec succeeds, and a stream of 3 channels (ldx > xlen) cut at {0, 1, an odd point, one before the input deficit, n} -- with
setphase on a seeded third of the cases -- gives, for every output of every channel,

    |y - ref| <= 2 (tp + 1) u absdot + 4 u_min          (per real component for complex signals)

with absdot = sum_k |h_k| |x_k| over the output's window, u = 2^-24 for Float32 arithmetic and 2^-53 whenever taps or signal are Float64,
u_min the smallest positive normal of that type (tests/test_polyphase_reference_cpu.py shows three subtly wrong kernels fail it).  The output
buffers start as NaN with ldy > nout: the tail stays NaN, the body has none, nwritten == outputlength; after every chunk (phi_idx, input_deficit)
equal the reference's and the history is bit-identical.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from fir_cases import CASES
from polyphase_ref import accumulation_unit, excess, outputlength, polyphase_ref

pytestmark = pytest.mark.gpu

NCH = 3
BUDGET = 1.5e7        # long-double multiply-adds of the reference per case (tp x outputs x channels, x2 complex): the file stays within minutes


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def stream_length(tp, L, M, nch, cplx, budget=BUDGET):
    """Samples per channel: several tiles where the reference's cost (budget long-double multiply-adds) allows, and always past the history and a few
    decimation steps.  mdsp_fir_kernel_path depends on it: tests/test_gpu_guard_misc.py takes its lengths from here too."""
    per_out = tp * nch * (2 if cplx else 1)
    return int(min(200_000, max(budget / per_out * M / L, tp + 4 * M + 300)))


def _case_id(c):
    L, M, hlen, td, xd, knobs, taps, path = c
    kn = "-".join(f"{k.replace('MDSP_FIR_', '').lower()}{v}" for k, v in knobs)
    return f"{L}_{M}_h{hlen}_{td}_{xd}{'_' + kn if kn else ''}{'_rsf' if taps == 'rsf' else ''}_p{path}"


def _taps(L, M, hlen, td, taps, rng):
    if taps == "rsf":
        from oracle import design
        h = np.asarray(design.resample_filter(Fraction(L, M)), dtype=np.float64)
        assert len(h) == hlen
    else:
        h = rng.standard_normal(hlen) / np.sqrt(max(1.0, hlen / L))
    return h.astype(np.float32 if td == "f32" else np.float64)


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_polyphase_path_against_extended_precision_reference(d, torch, case):
    from dsp_jl_amd import _lib
    from oracle import stream_filt as osf
    lib = _lib.lib()
    L, M, hlen, td, xd, knobs, taps, expect = case
    seed = L * 7919 + M * 104729 + hlen * 31 + len(knobs) * 7 + "f32 f64 c32 c64".index(xd)
    rng = np.random.default_rng(seed)
    h = _taps(L, M, hlen, td, taps, rng)
    xnp = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}[xd]
    lt = {"f32": _lib.F32, "f64": _lib.F64, "c32": _lib.C32, "c64": _lib.C64}
    cplx = xd[0] == "c"
    dbl = td == "f64" or xd in ("f64", "c64")
    ynp = (np.complex128 if dbl else np.complex64) if cplx else (np.float64 if dbl else np.float32)
    tdev = {np.float32: torch.float32, np.float64: torch.float64, np.complex64: torch.complex64, np.complex128: torch.complex128}
    rdt = np.float64 if dbl else np.float32
    tp = -(-hlen // L)
    n = stream_length(tp, L, M, NCH, cplx)
    x = rng.standard_normal((NCH, n))
    if cplx:
        x = x + 1j * rng.standard_normal((NCH, n))
    x = x.astype(xnp)
    ldx = n + 7
    xpad = np.zeros((NCH, ldx), dtype=xnp)
    xpad[:, :n] = x
    xd_dev = torch.from_numpy(xpad).to("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    u, umin = accumulation_unit(h.dtype, xnp)
    exact = dict(knobs).get("exact", 0)
    worst_ratio = 0.0
    fh = C.c_void_p()
    try:
        for k, v in knobs:
            if k != "exact":
                _lib.set_tunable(k, v)
        _lib.check(lib.mdsp_fir_create(C.byref(fh), h.ctypes.data_as(C.c_void_p), hlen, L, M, lt[td], lt[xd], NCH))
        if exact:
            _lib.check(lib.mdsp_fir_set_exact(fh, 1))
        of = osf.FIRFilter(h.astype(np.float64), Fraction(L, M))
        if seed % 3 == 0:                                            # setphase (resample's undelay! on half of them)
            phi = of.timedelay() if seed % 2 else float(rng.uniform(0, 3))
            of.setphase(phi)
            _lib.check(lib.mdsp_fir_setphase(fh, C.c_double(phi)))
        st_phi, st_def, hist = of.phi_idx, of.input_deficit, None
        path = C.c_int(-1)
        _lib.check(lib.mdsp_fir_kernel_path(fh, n, C.byref(path)))
        assert path.value == expect, f"kernel path {path.value}, the table says {expect}"
        odd = (n // 3) | 1
        hl = tp - 1
        a = 0
        for b in (0, 1, odd, None, n):
            if b is None:                                            # a chunk one sample short of the input deficit: no outputs, deficit 1
                b = odd + st_def - 1
            b = min(max(b, a), n)
            xlen = b - a
            nout = outputlength(xlen, L, M, st_phi, st_def)
            ol = C.c_int64()
            _lib.check(lib.mdsp_fir_outputlength(fh, xlen, C.byref(ol)))
            assert max(ol.value, 0) == nout                          # (the reference's formula: <= 0 for a chunk inside the deficit)
            ldy = nout + 5
            y = torch.full((NCH, ldy), complex(float("nan"), float("nan")) if cplx else float("nan"), dtype=tdev[ynp], device="cuda")
            nw = C.c_int64(-1)
            _lib.check(lib.mdsp_fir_exec(fh, xd_dev[:, a:].data_ptr(), xlen, ldx, y.data_ptr(), nout, ldy, C.byref(nw), stream))
            torch.cuda.synchronize()
            assert nw.value == nout
            yh = y.cpu().numpy()
            assert np.isnan(yh[:, nout:].view(rdt)).all()
            ref, ad, (st_phi, st_def, hist) = polyphase_ref(h, L, M, x[:, a:b], st_phi, st_def, hist)
            body = yh[:, :nout]
            assert not np.isnan(np.ascontiguousarray(body).view(rdt)).any()
            worst, ratio = excess(body, ref, ad, tp, u, umin)
            worst_ratio = max(worst_ratio, ratio)
            if worst > 1.0:
                err = np.abs(body.astype(ref.dtype) - ref)
                ch, m = np.unravel_index(int(np.argmax(err)), err.shape)
                pytest.fail(f"chunk [{a}, {b}): {worst:.3g} x the bound; worst output channel {ch} index {m} of {nout}: {body[ch, m]} vs {ref[ch, m]}")
            p_, d_ = C.c_int64(), C.c_int64()
            hd = np.empty((NCH, max(hl, 1)), dtype=xnp)
            _lib.check(lib.mdsp_fir_get_state(fh, C.byref(p_), C.byref(d_), hd.ctypes.data_as(C.c_void_p)))
            assert (p_.value, d_.value) == (st_phi, st_def), (a, b)
            if hl > 0:
                assert np.array_equal(hd.view(np.uint8), np.ascontiguousarray(hist).view(np.uint8)), (a, b)
            a = b
    finally:
        if fh.value:
            _lib.check(lib.mdsp_fir_destroy(fh))
        for k, v in knobs:
            if k != "exact":
                _lib.set_tunable(k, None)
    print(f"\nmargin path={expect} taps={td} x={xd} L={L} M={M} tp={tp} max|y-ref|/(u absdot)={worst_ratio:.3f} bound/(u absdot)={2 * (tp + 1)}")
