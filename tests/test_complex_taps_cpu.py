"""CPU checks for complex FIR taps:

  1. tests/complex_taps_ref.py, the extended-precision reference of the GPU sweep (tests/test_gpu_complex_taps.py), agrees with the oracle
     (oracle.stream_filt.FIRFilter, generic in the tap dtype) on every row of tests/complex_tap_cases.py -- within the sweep's bound at the
     oracle's precision, with bit-identical state after every chunk;
  2. that bound, |y - ref| <= 2 (n + 1) u absdot + 4 u_min per real component, fails four deliberately wrong evaluations on every row
     (conjugated taps, imaginary part of the taps dropped, sign of the h_im x_im term flipped, real and imaginary outputs swapped): it is not
     vacuous;
  3. without a device, FIRFilter with complex taps constructs and its host state follows the oracle's; DF2TFilter with complex b is refused
     by the missing device only; FIRArbitrary with complex taps stays UnsupportedError;
  4. the argument errors of filt(b, a, x) come before any device work for complex inputs too.
"""
from fractions import Fraction

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
from oracle import stream_filt as osf

from complex_tap_cases import CASES
from complex_taps_ref import accumulation_unit, complex_taps_ref, excess, terms

NP = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}


def case_id(c):
    L, M, hlen, td, xd, knobs, taps, path = c
    return f"{L}_{M}_h{hlen}_{td}_{xd}{'_exact' if knobs else ''}{'_rsf' if taps == 'rsf' else ''}_p{path}"


def case_taps(L, M, hlen, td, taps, rng):
    """The row's taps: seeded complex normal ones, or the default resampling filter shifted to a channel centre."""
    if taps == "rsf":
        from oracle import design
        h = np.asarray(design.resample_filter(Fraction(L, M)), dtype=np.float64)
        assert len(h) == hlen
        h = h * np.exp(2j * np.pi * 0.1 * np.arange(hlen) / L)
    else:
        h = (rng.standard_normal(hlen) + 1j * rng.standard_normal(hlen)) / np.sqrt(max(1.0, hlen / L))
    return h.astype(NP[td])


def case_signal(xd, shape, rng):
    x = rng.standard_normal(shape)
    if xd[0] == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(NP[xd])


def _setup(case):
    L, M, hlen, td, xd, knobs, taps, _ = case
    rng = np.random.default_rng(L * 7919 + M * 104729 + hlen * 31 + "f32 f64 c32 c64".index(xd) + 5 * (td == "c64"))
    h = case_taps(L, M, hlen, td, taps, rng)
    tp = -(-hlen // L)
    n = tp + 3 * M + int(rng.integers(20, 60))          # past the history and a few decimation steps; the oracle is a Python loop per output
    if L > 8:
        n = max(8, min(n, 4000 // L))
    return L, M, hlen, h, tp, case_signal(xd, n, rng), rng


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_reference_equals_the_oracle_on_every_case(case):
    L, M, hlen, h, tp, x, rng = _setup(case)
    n = len(x)
    wide = np.complex128 if x.dtype.kind == "c" else np.float64
    of = osf.FIRFilter(h.astype(np.complex128), Fraction(L, M))
    if (L, M) != (1, 1) and hlen % 3 == 0:
        of.setphase(float(rng.uniform(0, 3)))
    phi, dfc, hist = of.phi_idx, of.input_deficit, None
    cuts = sorted({0, 1, n // 3 | 1, n} & set(range(n + 1)))
    for a, b in zip([0] + cuts, cuts):
        yo = of.filt(x[a:b].astype(wide))
        y, ad, (phi, dfc, hist) = complex_taps_ref(h, L, M, x[a:b], phi, dfc, hist)
        assert (phi, dfc) == (of.phi_idx, of.input_deficit), (a, b)
        assert np.array_equal(hist.astype(wide), of.history), (a, b)
        assert y.shape == yo.shape and yo.dtype == np.complex128
        if y.size:
            worst, _ = excess(yo, y, ad, terms(tp, x.dtype), 2.0 ** -53, float(np.finfo(np.float64).tiny))
            assert worst <= 1.0, (a, b, worst)


def _eval(h, L, M, x, dtype, wrong=None):
    """One chunk from zero state in the arithmetic `dtype` (complex64 / complex128), oldest sample first; `wrong` picks a faulty variant."""
    pfb = osf.taps2pfb(h, L).astype(dtype)
    if wrong == "conjugated taps":
        pfb = np.conj(pfb)
    elif wrong == "imaginary part of the taps dropped":
        pfb = pfb.real.astype(dtype)
    tp = pfb.shape[0]
    z = np.concatenate([np.zeros(tp - 1, dtype=x.dtype), x]).astype(dtype)
    nout = -(-(len(x) * L) // M)
    phi, idx = osf.polyphase_closed_form(1, 1, L, M, np.arange(nout))
    acc = np.zeros(nout, dtype=dtype)
    for k in range(tp):
        hk, zk = pfb[k, phi - 1], z[idx - 1 + k]
        if wrong == "sign of the h_im x_im term flipped":
            acc = acc + ((hk.real * zk.real + hk.imag * zk.imag) + 1j * (hk.real * zk.imag + hk.imag * zk.real)).astype(dtype)
        else:
            acc = (acc + (hk * zk).astype(dtype)).astype(dtype)
    if wrong == "real and imaginary outputs swapped":
        acc = (acc.imag + 1j * acc.real).astype(dtype)
    return acc


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_the_bound_passes_a_correct_evaluation_and_fails_four_wrong_ones(case):
    L, M, hlen, h, tp, x, _ = _setup(case)
    td, xd = case[3], case[4]
    u, umin = accumulation_unit(NP[td], NP[xd])
    dtype = np.complex128 if u < 1e-10 else np.complex64
    y, ad, _ = complex_taps_ref(h, L, M, x)
    n = terms(tp, x.dtype)
    worst, _ = excess(_eval(h, L, M, x, dtype), y, ad, n, u, umin)
    assert worst <= 1.0, worst
    wrongs = ["conjugated taps", "imaginary part of the taps dropped", "real and imaginary outputs swapped"]
    if x.dtype.kind == "c":
        wrongs.append("sign of the h_im x_im term flipped")       # (a real signal has no x_im: the term does not exist)
    for what in wrongs:
        assert excess(_eval(h, L, M, x, dtype, what), y, ad, n, u, umin)[0] > 1.0, what


# --- 3: the host objects, without a device ----------------------------------------------------------------------------------------------------

def test_firfilter_with_complex_taps_constructs_and_its_host_state_matches_the_oracle():
    rng = np.random.default_rng(50)
    for k in range(300):
        ratio = Fraction(int(rng.integers(1, 11)), int(rng.integers(1, 11)))
        hlen = int(rng.integers(1, 101))
        dt = (np.complex64, np.complex128)[k % 2]
        h = (rng.standard_normal(hlen) + 1j * rng.standard_normal(hlen)).astype(dt)
        a, b = d.FIRFilter(h, ratio), osf.FIRFilter(h, ratio)
        assert a.h.dtype == np.dtype(dt) and np.array_equal(a.h, h)
        assert a.kernel.lower().endswith(b.kind)
        assert a.tapsPerphi == getattr(b, "taps_per_phi", b.hlen)
        if ratio != 1:
            ph = 10 * rng.random()
            a.setphase(ph); b.setphase(ph)
        assert (a.phi_idx, a.input_deficit, a.historyLen) == (b.phi_idx, b.input_deficit, b.history_len)
        assert a.timedelay() == b.timedelay()
        yl = int(rng.integers(1, 101))
        assert a.inputlength(yl) == b.inputlength(yl) and a.inputlength(yl, True) == b.inputlength(yl, True)
        assert a.outputlength(yl) == b.outputlength(yl)
    # anything else complex is widened to ComplexF64
    assert d.FIRFilter(np.array([1 + 2j, 3], dtype=np.clongdouble), 2).h.dtype == np.dtype(np.complex128)


def test_complex_coefficients_are_refused_by_the_missing_device_only():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    b = np.array([1 + 1j, 2 - 1j, 0.5j])
    with pytest.raises(d.DeviceError):
        d.DF2TFilter(b)
    with pytest.raises(d.DeviceError):
        d.DF2TFilter(b.astype(np.complex64), 2.0 + 1j)
    with pytest.raises(d.DeviceError):
        d.filt(b, 1.0, np.ones(8))
    with pytest.raises(d.DeviceError):
        d.tdfilt(b, np.ones(8))
    with pytest.raises(d.DeviceError):
        d.filtfilt(b, np.ones(8))
    with pytest.raises(d.DeviceError):
        d.FIRFilter(b, Fraction(3, 2)).filt(np.ones(8))


def test_firarbitrary_with_complex_taps_stays_unsupported():
    with pytest.raises(d.UnsupportedError, match="FIRArbitrary"):
        d.FIRFilter(np.array([1 + 1j, 2 - 1j, 0.5j]), 1.37)
    with pytest.raises(d.UnsupportedError, match="FIRArbitrary"):
        d.FIRFilter(np.ones(5, dtype=np.complex64), np.float64(0.5), 16)


# --- 4: argument errors before device work ----------------------------------------------------------------------------------------------------

def test_argument_errors_of_filt_come_before_device_work_for_complex_inputs():
    x = np.ones(4, dtype=np.complex64)
    with pytest.raises(d.ArgumentError):
        d.filt(np.array([], dtype=np.complex128), 1.0, x)                       # dspbase.jl:28
    with pytest.raises(d.ArgumentError):
        d.filt(np.array([1 + 1j, 2]), 0.0 + 0.0j, x)                            # dspbase.jl:30
    with pytest.raises(d.ArgumentError):
        d.filt(np.array([1 + 1j, 2]), np.array([], dtype=np.complex64), x)
    with pytest.raises(d.UnsupportedError):
        d.filt(np.array([1 + 1j, 2]), np.array([1.0, 0.5j]), x)                 # IIR stays as it is
    with pytest.raises(d.ArgumentError):
        d.DF2TFilter(np.array([1 + 1j, 2]), 0.0)
    with pytest.raises(d.UnsupportedError):
        d.filtfilt(np.array([1 + 1j, 2]), np.array([1.0, 0.5]), np.ones(8))     # IIR stays as it is
    with pytest.raises(TypeError):
        d.fftfilt(np.array([1 + 1j, 2]), np.ones(8))                            # fftfilt stays real-only
