"""The 2-D periodogram on the device (periodograms.jl:473-509): DSP.jl's own tests (test/periodograms.jl:262-329) and docstring examples
(:449-471), then every route against the Float64 reference of tests/periodogram2_ref.py.

Bounds.  Each power value is |X|^2 / r of a 2-D transform of N1 N2 points.  Norm-wise: ||got - ref|| / ||ref|| <= 4 log2(N1 N2) u;
element-wise: max |got - ref| <= 8 log2(N1 N2) u max |ref| ("ulps of the max": a transform's rounding error scales with the signal's
energy, not with each bin's value), u = 2^-24 for Float32 input and 2^-53 otherwise.
Radial bin k sums wc_k weighted powers.  By Cauchy-Schwarz the transform error it collects is at most 8 log2(N1 N2) u sqrt(R_k E) (R_k the
radialsum value, E the total energy sum |X|^2 / r), and its Float64 sum over wc_k terms adds wc_k 2^-53 R_k; radialavg divides both by wc_k.
Norm-wise: 4 log2(N1 N2) u + max(wc) 2^-53.
"""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
from dsp_jl_amd.periodograms import _P2Plan

from conftest import isapprox
from periodogram2_ref import periodogram2_ref, wave_counts
from test_periodogram2_cpu import sparse_radial_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def per2d():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per2d_golden.npz"))


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def check_bounds(got, ref, N1, N2, dtype):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    lg = np.log2(N1 * N2)
    got = _np(got).astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    nrm = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    ulp = np.max(np.abs(got - ref)) / (u * np.max(np.abs(ref)))
    assert nrm <= 4 * lg * u, (nrm, 4 * lg * u)
    assert ulp <= 8 * lg, (ulp, 8 * lg)


def check_radial(got, ref, x64, N1, N2, dtype, avg):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    lg = np.log2(N1 * N2)
    got = _np(got).astype(np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    wc = wave_counts(N1, N2)[1].astype(np.float64)
    R = ref * wc if avg else ref
    E = np.sum(x64 ** 2) * N1 * N2 / x64.size                  # Parseval: sum |X|^2 / (n1 n2)
    bound = 8 * lg * u * np.sqrt(R * E) + wc * 2.0 ** -53 * R
    if avg:
        bound = bound / wc
    err = np.abs(got - ref)
    assert np.all(err <= bound), (np.max(err / bound), np.argmax(err / bound))
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) <= 4 * lg * u + np.max(wc) * 2.0 ** -53


# ---- DSP.jl's tests and examples -----------------------------------------------------------------------------------------------------------
def test_octave_goldens(per2d):
    x = per2d["per2dx"]
    assert isapprox(d.power(d.periodogram(x, fs=1, radialsum=True)), per2d["per2dsum"])       # test/periodograms.jl:275
    assert isapprox(d.power(d.periodogram(x, fs=1, radialavg=True)), per2d["per2dmean"])      # :280


def test_full_psd_and_padding(per2d):
    x = per2d["per2dx"]
    p = d.periodogram(x, fs=1)
    assert isinstance(p, d.Periodogram2)
    assert isapprox(d.power(p), np.abs(np.fft.fft2(x)) ** 2 / x.size)                        # :283
    pads = (x.shape[0] + 4, x.shape[0] + 7)
    xp = np.zeros(pads)
    xp[:x.shape[0], :x.shape[1]] = x
    assert isapprox(d.power(d.periodogram(x, fs=1, nfft=pads)), np.abs(np.fft.fft2(xp)) ** 2 / x.size)   # :289


def test_docstring_examples():
    pxx = d.periodogram(np.array([[1, 1], [0, 1], [0, 0]]), nfft=(3, 2))                    # periodograms.jl:449-460
    assert isapprox(d.power(pxx), np.array([[1.5, 1 / 6], [0.5, 1 / 6], [0.5, 1 / 6]]))
    assert d.power(pxx).dtype == np.float64
    f1, f2 = d.freq(pxx)
    assert np.allclose(f1, [0.0, 1 / 3, -1 / 3]) and np.allclose(f2, [0.0, -0.5])
    x = np.array([[1, 3], [0, 1]])
    ps = d.periodogram(x, radialsum=True)                                                     # :462-471
    assert isinstance(ps, d.Periodogram)
    assert isapprox(d.power(ps), [6.25, 4.75]) and np.allclose(d.freq(ps), [0.0, 0.5])
    pa = d.periodogram(x, radialavg=True)
    assert isapprox(d.power(pa), [6.25, 1.5833333333333333]) and np.allclose(d.freq(pa), [0.0, 0.5])


def test_freq_and_fftshift(per2d):
    x = per2d["per2dx"]
    assert isapprox(d.freq(d.periodogram(x, fs=3.3, radialsum=True)), d.freq(d.periodogram(x[0, :].copy(), fs=3.3)))   # :291
    f1, f2 = d.freq(d.periodogram(x, fs=3.3))                                                 # :293-301
    f1d = d.freq(d.periodogram(x[0, :].copy(), fs=3.3, onesided=False))
    assert np.allclose(f1, f1d) and np.allclose(f2, f1d)
    p = d.periodogram(x)                                                                      # :302-307
    ps = d.fftshift(p)
    assert np.array_equal(np.fft.fftshift(d.power(p)), d.power(ps))
    assert d.fftshift(ps) is ps
    f = d.freq(p)
    assert all(np.array_equal(a, b) for a, b in zip((np.fft.fftshift(f[0]), np.fft.fftshift(f[1])), d.freq(ps)))
    pd = d.fftshift(d.periodogram(torch.from_numpy(x).cuda()))                               # device power shifts on the device
    assert isinstance(pd.power, torch.Tensor) and np.array_equal(_np(pd.power), d.power(ps))


@pytest.mark.parametrize("shape", [(52, 46), (46, 52)])
def test_sparse_radial_case(shape):
    y, pe, fwn, f = sparse_radial_case(52, 46)                                                # test/periodograms.jl:310-329
    if shape[0] < shape[1]:
        y = y.T                                                                                # the other c1 / c2 branch
    P = d.periodogram(y, nfft=shape, radialsum=True)
    assert isapprox(d.power(P), pe)
    assert np.isclose(d.freq(P)[fwn], f)


# ---- every route against the Float64 reference ---------------------------------------------------------------------------------------------
RNG = np.random.default_rng(20261015)
F, R, A = d.ENGINE_FUSED, d.ENGINE_ROCFFT, d.ENGINE_AUTO
CASES = [   # (n1, n2, nfft or None, input dtype, engine, device input)
    (32, 32, None, np.float32, F, True), (32, 32, None, np.float64, R, False), (33, 31, None, np.int64, A, False),
    (2, 64, None, np.float32, A, True), (2, 63, (2, 64), np.float64, F, True), (3, 5, None, np.float64, A, True),
    (100, 60, (105, 63), np.float32, A, False), (45, 77, None, np.float32, R, True), (127, 255, (128, 256), np.float64, F, False),
    (256, 256, None, np.float32, F, True), (256, 256, None, np.float64, R, True), (480, 300, None, np.float32, R, False),
    (1000, 999, None, np.float64, A, True), (1024, 768, None, np.float32, F, False), (3000, 2000, None, np.float32, F, True),
    (3000, 2000, None, np.float32, R, True), (3000, 2000, None, np.float64, A, True), (2048, 2048, None, np.float64, F, True),
    (4096, 4096, None, np.float32, A, True), (8192, 4096, None, np.float32, A, True),
    (8, 70000, None, np.float32, A, True), (140000, 4, None, np.float64, A, True),
]


def _input(n1, n2, dt):
    if np.dtype(dt).kind == "i":
        return RNG.integers(-50, 50, size=(n1, n2)).astype(dt)
    return np.asfortranarray(RNG.standard_normal((n1, n2)) + 0.25).astype(dt)


@pytest.mark.parametrize("n1,n2,nfft,dt,eng,dev", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{np.dtype(c[3]).name}-e{c[4]}-{'dev' if c[5] else 'host'}" for c in CASES])
def test_against_reference(n1, n2, nfft, dt, eng, dev):
    x = _input(n1, n2, dt)
    N1, N2 = nfft if nfft else d.nextfastfft((n1, n2))
    T = d.fftabs2type(d.fftintype(x.dtype))
    s = torch.from_numpy(np.ascontiguousarray(x)).cuda() if dev else x
    full = d.periodogram(s, nfft=nfft, engine=eng) if nfft else d.periodogram(s, engine=eng)
    assert isinstance(full.power, torch.Tensor) == dev
    assert full.power.shape == (N1, N2) and _np(full.power).dtype == T
    if dev:
        assert full.power.stride() == (1, N1)                   # first axis contiguous, like the Julia matrix
    x64 = x.astype(np.float64)
    check_bounds(full.power, periodogram2_ref(x64, (N1, N2)), N1, N2, T)
    if n1 * n2 > 16_000_000:
        return                                                  # the radial forms of the largest shapes: test_radial_large
    for kw in ({"radialsum": True}, {"radialavg": True}):
        p = d.periodogram(s, nfft=(N1, N2), engine=eng, **kw)
        assert _np(p.power).dtype == T
        check_radial(p.power, periodogram2_ref(x64, (N1, N2), **kw), x64, N1, N2, T, "radialavg" in kw)


def test_radial_large():
    x = _input(4096, 4096, np.float32)
    s = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    x64 = x.astype(np.float64)
    for kw in ({"radialsum": True}, {"radialavg": True}):
        check_radial(d.periodogram(s, **kw).power, periodogram2_ref(x64, (4096, 4096), **kw), x64, 4096, 4096, np.float32, "radialavg" in kw)


# ---- plan-level properties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", [0, 1, 2])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_bitwise_reproducible(ptype, dt):
    x = torch.from_numpy(_input(1500, 1100, dt)).cuda()
    kw = [{}, {"radialsum": True}, {"radialavg": True}][ptype]
    a = d.periodogram(x, **kw).power.clone()
    b = d.periodogram(x, **kw).power
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_output_stride_keeps_the_tail():
    n1, n2, N1, N2, ldo = 30, 20, 36, 21, 41
    x = _input(n1, n2, np.float64)
    plan = _P2Plan(n1, n2, N1, N2, 1.0, 0, np.float64, d.ENGINE_AUTO)
    assert plan.nout == N1 * N2 and plan.workspace_bytes > 0
    s = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()      # (n2, n1): column j of x contiguous
    out = torch.full((N2, ldo), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().mdsp_periodogram2_exec(plan._h, s.data_ptr(), n1, out.data_ptr(), ldo, torch.cuda.current_stream().cuda_stream))
    o = out.cpu().numpy()
    assert np.all(o[:, N1:] == -7.0)
    check_bounds(o[:, :N1].T.copy(), periodogram2_ref(x, (N1, N2)), N1, N2, np.float64)
    ref = np.asarray(d.power(d.periodogram(x, nfft=(N1, N2))))
    assert np.array_equal(o[:, :N1].T, ref)                     # the same plan arithmetic as the function-style call


def test_engine_reported_and_lds_checked():
    plan = _P2Plan(64, 64, 64, 64, 1.0, 1, np.float32, d.ENGINE_ROCFFT)
    assert plan.engine == d.ENGINE_ROCFFT and plan.nout == 33
    s = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    out = torch.zeros(33, dtype=torch.float32, device="cuda")
    assert _lib.lib().mdsp_periodogram2_exec(plan._h, s.data_ptr(), 63, out.data_ptr(), 1, None) == _lib.ERR_DIMENSION
    wc = np.zeros(33, dtype=np.int64)
    k = C.c_int64()
    _lib.check(_lib.lib().mdsp_periodogram2_geometry_for(64, 64, C.byref(k), wc.ctypes.data_as(C.POINTER(C.c_int64)), None))
    assert k.value == 33 and np.all(wc > 0)


def test_complex_matrix_keeps_the_columnwise_method():
    """Complex 2-D input is unchanged: one PSD per column (the pre-existing behaviour)."""
    x = (RNG.standard_normal((64, 3)) + 1j * RNG.standard_normal((64, 3))).astype(np.complex64)
    p = d.periodogram(x)
    assert p.power.shape == (64, 3)
    assert np.array_equal(p.power, d.stft(x, 64, 0, True, onesided=False)[:, 0])
