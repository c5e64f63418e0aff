"""CPU checks of the 2-D periodogram (periodograms.jl:473-509): the Float64 reference against DSP.jl's own golden vectors, the library's
radial geometry (mdsp_periodogram2_geometry_for) against the reference's index loop, and the argument errors, raised before any device
work (so they are the same on a machine without a GPU)."""
import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
from dsp_jl_amd.periodograms import periodogram2_geometry

from conftest import isapprox
from periodogram2_ref import periodogram2_ref, radial_bins, wave_counts


@pytest.fixture(scope="module")
def per2d():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per2d_golden.npz"))


def sparse_radial_case(n1=52, n2=46, nf=(22, 7)):
    """test/periodograms.jl:310-329: a real signal with one conjugate pair of non-zero 2-D Fourier coefficients; returns (y, expected
    radialsum, the 0-based bin of the pair, the frequency of that bin).  n1 < n2 (the transposed case) takes the other c1 / c2 branch."""
    F = (np.fft.fftfreq(n1), np.fft.fftfreq(n2))
    a = np.array([F[0][nf[0] - 1], F[1][nf[1] - 1]])
    x = np.zeros((n1, n2), dtype=np.complex128)
    for i in range(n1):
        for j in range(n2):
            f = np.array([F[0][i], F[1][j]])
            if np.array_equal(f, a):
                x[i, j] = 1 + 2j
            elif np.array_equal(f, -a):
                x[i, j] = 1 - 2j
    y = np.real(np.fft.ifft2(x))
    nmin = min(n1, n2)
    fwn = int(np.rint(np.sqrt(a[0] ** 2 + a[1] ** 2) * nmin))
    pe = np.zeros((nmin >> 1) + 1)
    pe[fwn] = 2 * abs(x[nf[0] - 1, nf[1] - 1]) ** 2 / n1 / n2
    return y, pe, fwn, fwn / nmin


# ---- the reference restatement against the reference's goldens -------------------------------------------------------------------------
def test_reference_reproduces_the_octave_goldens(per2d):
    x = per2d["per2dx"]
    assert isapprox(periodogram2_ref(x, radialsum=True), per2d["per2dsum"])          # test/periodograms.jl:275
    assert isapprox(periodogram2_ref(x, radialavg=True), per2d["per2dmean"])         # :280
    assert isapprox(periodogram2_ref(x), np.abs(np.fft.fft2(x)) ** 2 / x.size)        # :283


@pytest.mark.parametrize("shape", [(52, 46), (46, 52)])
def test_reference_sparse_radial_case(shape):
    if shape[0] > shape[1]:
        y, pe, fwn, f = sparse_radial_case(*shape)
    else:                                  # the transpose: nfft = (46, 52), the pair at the transposed index
        y, pe, fwn, f = sparse_radial_case(52, 46)
        y = y.T
    got = periodogram2_ref(y, nfft=y.shape, radialsum=True)
    assert isapprox(got, pe)
    assert np.argmax(got) == fwn


# ---- the library's geometry against the reference's loop --------------------------------------------------------------------------------
def _loop_geometry(n1, n2):
    wavenum, kmax, _ = radial_bins(n1, n2)
    widths = sum(len(np.unique(row[row <= kmax])) for row in wavenum)
    return kmax, wave_counts(n1, n2)[1], int(widths)


def test_geometry_matches_the_reference_loop_small():
    for n1 in range(2, 65):
        for n2 in range(2, 65):
            kmax, wc, parts = periodogram2_geometry(n1, n2)
            k2, wc2, p2 = _loop_geometry(n1, n2)
            assert kmax == k2 == min(n1, n2) // 2 + 1, (n1, n2)
            assert np.array_equal(wc, wc2), (n1, n2, wc, wc2)
            assert parts == p2, (n1, n2, parts, p2)


@pytest.mark.parametrize("n1,n2", [(1000, 1000), (999, 1001), (1001, 640), (2, 3000), (3001, 7), (1536, 1025), (700, 2100), (4096, 8)])
def test_geometry_matches_the_reference_loop_large(n1, n2):
    kmax, wc, parts = periodogram2_geometry(n1, n2)
    k2, wc2, p2 = _loop_geometry(n1, n2)
    assert kmax == k2 and np.array_equal(wc, wc2) and parts == p2


def test_geometry_rejects_degenerate_sizes():
    with pytest.raises(d.ArgumentError):
        periodogram2_geometry(1, 8)


# ---- argument errors before device work --------------------------------------------------------------------------------------------------
def test_argument_errors_before_device_work():
    s = np.ones((4, 5))
    with pytest.raises(d.ArgumentError, match="nfft must be >= size"):
        d.periodogram(s, nfft=(3, 5))                                     # :477
    with pytest.raises(d.ArgumentError, match="nfft must be >= size"):
        d.periodogram(s, nfft=(4, 4))
    with pytest.raises(d.ArgumentError, match="dimensions"):
        d.periodogram(np.ones((1, 5)))                                    # :478
    with pytest.raises(d.ArgumentError, match="dimensions"):
        d.periodogram(np.ones((6, 1)), nfft=(8, 8))
    with pytest.raises(d.ArgumentError, match="mutually exclusive"):
        d.periodogram(s, radialsum=True, radialavg=True)                  # :480


def test_type_errors_before_device_work():
    s = np.ones((4, 5))
    with pytest.raises(TypeError):
        d.periodogram(s, nfft=8)                                          # nfft::NTuple{2,Int}
    with pytest.raises(TypeError):
        d.periodogram(s, nfft=(8.0, 8))
    with pytest.raises(TypeError):
        d.periodogram(s, onesided=True)                                   # the matrix method has no onesided / window
    with pytest.raises(TypeError):
        d.periodogram(s, window=None)
    with pytest.raises(TypeError):
        d.periodogram(np.ones(16), radialsum=True)                        # the vector method has no radialsum / radialavg
    with pytest.raises(TypeError):
        d.periodogram(np.ones(16), radialavg=False)


def test_c_plan_checks_in_the_reference_order():
    """The C entry checks its arguments before it touches the device (the same status with and without a GPU)."""
    import ctypes as C
    lib = _lib.lib()
    h = C.c_void_p()
    cases = [((4, 5, 3, 5, 1.0, 0, _lib.F64), "nfft must be >= size(s)"),
             ((1, 5, 1, 5, 1.0, 0, _lib.F64), "dimensions of s must be > 1"),
             ((4, 5, 4, 5, 1.0, 3, _lib.F64), "ptype"),
             ((4, 5, 4, 5, 1.0, 0, _lib.C64), "real matrix"),
             ((4, 5, 3, 5, 1.0, 7, _lib.C64), "nfft must be >= size(s)")]      # the first failing check wins
    for args, msg in cases:
        assert lib.mdsp_periodogram2_plan_create(C.byref(h), *args, _lib.ENGINE_AUTO) == _lib.ERR_ARGUMENT
        assert msg in lib.mdsp_last_error_string().decode()
        assert not h.value


def test_periodogram2_result_type_and_fftshift_on_the_host():
    """Periodogram2, freq and fftshift (periodograms.jl:284-288, :330-339; test/periodograms.jl:258-263) need no device."""
    p = d.Periodogram2(np.array([[1, 2], [3, 4]]), np.arange(1, 3), np.fft.fftfreq(2))
    ps = d.fftshift(p)
    assert np.array_equal(ps.power, np.fft.fftshift(p.power, 1))
    assert np.array_equal(ps.freq1, p.freq1) and np.array_equal(ps.freq2, np.fft.fftshift(p.freq2))
    f1, f2 = d.freq(p)
    assert f1 is p.freq1 and f2 is p.freq2
    assert d.power(p) is p.power
    q = d.Periodogram2(np.arange(12.0).reshape(3, 4), np.fft.fftfreq(3), np.fft.fftfreq(4))
    qs = d.fftshift(q)
    assert np.array_equal(qs.power, np.fft.fftshift(q.power))
    assert np.array_equal(qs.freq1, np.fft.fftshift(q.freq1)) and np.array_equal(qs.freq2, np.fft.fftshift(q.freq2))
    assert d.fftshift(qs) is qs                                            # already shifted: returned as it is
