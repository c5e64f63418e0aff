"""Biquad / SecondOrderSections filtering on the device: mdsp_sos_exec equals the host emulation bit for bit (every length at which the tiling takes
another path, both cuts, section counts on both sides of the compiled sizes, all four working types, padded columns, both directions, in place, a
start state in and the end state out), and the public calls -- filt, filt_, DF2TFilter, filtfilt -- agree with the numpy restatements of the
reference (tests/sos_ref.py) under the bound of tests/test_sos_cpu.py."""
import numpy as np
import pytest

import sos_cases as sc
import sos_ref as sr

pytestmark = pytest.mark.gpu

C_BOUND = 8.0          # tests/test_sos_cpu.py: twice the worst measured e_scan / e_serial, rounded up to a power of two
TYPES = (np.float32, np.float64, np.complex64, np.complex128)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _rows(K):
    return {1: sc.table("butter2_02"), 2: (sc.table("butter8_02")[0][:2], 0.25), 3: sc.table("butter5_02"),
            5: (sc.table("butter32_02")[0][:5], 0.0625), 16: sc.table("butter32_02")}[K]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _real(dt):
    return np.dtype(np.float32) if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


@pytest.mark.parametrize("dt", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("gain", [True, False], ids=["gain", "nogain"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 16])
def test_exec_equals_the_host_emulation_bit_for_bit(d, K, gain, dt):
    import torch
    tb, g = _rows(K)
    g = g if gain else None
    _, _, tile, P, _ = d.sos_geometry(K, dt, 1, 1)
    for n in (1, 2, P - 1, P, P + 1, tile - 1, tile, tile + 1, 2 * tile + 3):
        for segments in (1, 3):
            for ncols, ld in ((1, n), (3, n + 5)):
                plan = d.SosPlan(tb, g, dt, n, ncols, segments)
                assert plan.segments == min(segments, n)
                x = np.zeros((ncols, ld), dt)
                x[:, :n] = sc.signal(n, ncols, dt, salt=n + K).reshape(n, ncols).T
                st0 = (0.1 * sc.signal(2 * K, ncols, dt, salt=n + 1)).reshape(2, K, ncols)
                for reverse in (False, True):
                    what = f"K {K} n {n} segments {segments} ncols {ncols} reverse {reverse}"
                    want, st_want = sc.emulate(tb, g, x[:, :n].T, dt, segments, state=st0, reverse=reverse)
                    want = np.asarray(want).reshape(n, ncols).T
                    xd, yd = torch.from_numpy(x).cuda(), torch.zeros((ncols, ld), dtype=torch.from_numpy(x).dtype, device="cuda")
                    sd = torch.from_numpy(np.ascontiguousarray(st0.transpose(2, 1, 0))).cuda()
                    plan.exec(xd.data_ptr(), ld, yd.data_ptr(), ld, sd.data_ptr(), reverse)
                    got, st_got = yd.cpu().numpy(), sd.cpu().numpy().transpose(2, 1, 0)
                    assert np.array_equal(_bits(got[:, :n]), _bits(want)), what
                    assert np.array_equal(_bits(st_got), _bits(st_want)), what + " (end state)"
                    assert not got[:, n:].any(), what + " (padding written)"
                    sd = torch.from_numpy(np.ascontiguousarray(st0.transpose(2, 1, 0))).cuda()
                    plan.exec(xd.data_ptr(), ld, xd.data_ptr(), ld, sd.data_ptr(), reverse)       # in place
                    assert np.array_equal(_bits(xd.cpu().numpy()[:, :n]), _bits(want)), what + " in place"
                    assert np.array_equal(_bits(sd.cpu().numpy().transpose(2, 1, 0)), _bits(st_want)), what + " in place (end state)"
                # no state: zero start, end state dropped
                want, _ = sc.emulate(tb, g, x[:, :n].T, dt, segments)
                xd, yd = torch.from_numpy(x).cuda(), torch.zeros((ncols, ld), dtype=torch.from_numpy(x).dtype, device="cuda")
                plan.exec(xd.data_ptr(), ld, yd.data_ptr(), ld)
                assert np.array_equal(_bits(yd.cpu().numpy()[:, :n]), _bits(np.asarray(want).reshape(n, ncols).T)), f"K {K} n {n} no state"
    torch.cuda.synchronize()


def _plan_run(d, rows, gain, x, dt, segments, reverse=False):
    """The (n, ncols) array x through a SosPlan with the cut forced; returns the filtered array."""
    import torch
    n, ncols = x.shape
    plan = d.SosPlan(rows, gain, dt, n, ncols, segments)
    assert plan.segments == min(segments, n)
    xd = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    yd = torch.empty_like(xd)
    plan.exec(xd.data_ptr(), n, yd.data_ptr(), n, None, reverse)
    return yd.cpu().numpy().T


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("segments", [1, 3])
def test_exact_integer_cases_on_the_device(d, dt, segments):
    """No tolerance: the integrator is a cumulative sum, the FIR-only biquad the integer convolution, an identity cascade returns x -- at every length
    of the bit-equality test, in one launch and through reduce / carries / apply."""
    _, _, tile, P, _ = d.sos_geometry(1, dt, 1, 1)
    for n in (1, 2, P - 1, P, P + 1, tile - 1, tile, tile + 1, 2 * tile + 3):
        x = sc.small_integers(n, 2, dt, salt=n).reshape(n, 2)
        assert np.array_equal(_plan_run(d, [sc.INTEGRATOR], None, x, dt, segments), np.cumsum(x, axis=0, dtype=np.float64).astype(dt)), ("integrator", n)
        assert np.array_equal(_plan_run(d, [sc.INTEGRATOR], None, x, dt, segments, reverse=True),
                              np.cumsum(x[::-1], axis=0, dtype=np.float64)[::-1].astype(dt)), ("integrator reversed", n)
        conv = np.stack([np.convolve(x[:, c].astype(np.float64), [1.0, 2.0, 3.0])[:n] for c in range(2)], axis=1).astype(dt)
        assert np.array_equal(_plan_run(d, [sc.FIR_ONLY], None, x, dt, segments), conv), ("fir", n)
        xr = sc.signal(n, 2, dt, salt=n).reshape(n, 2)
        assert np.array_equal(_plan_run(d, [sc.IDENTITY] * 3, 1.0, xr, dt, segments), xr), ("identity", n)
    # and through the public call
    x = sc.small_integers(tile + 1, 2, dt)
    assert np.array_equal(d.filt(d.Biquad(*sc.INTEGRATOR), x), np.cumsum(x, axis=0, dtype=np.float64).astype(dt))


def test_an_automatically_cut_column(d):
    """16 tiles in one column: the automatic cut gives four segments on tile boundaries, so the public call takes reduce / carries / apply.  Column 0
    against the restatement under the bound; a NaN in column 1 behind a segment boundary: the samples before it as without it, the restatement's mask
    from it on, column 0 untouched."""
    dt = np.float32
    tb, g = sc.table("butter5_02")
    _, _, tile, P, _ = d.sos_geometry(len(tb), dt, 1, 1)
    n = 16 * tile
    S, seglen, _, _, _ = d.sos_geometry(len(tb), dt, n, 2)
    assert S == 4 and seglen == 4 * tile
    f = _sos(d, coef_dtype=dt)
    x = sc.signal(n, 2, dt)
    ref, _ = sr.sos_filt(tb, g, x, np.longdouble)
    ser, _ = sr.sos_filt(tb, g, x, dt)
    clean = d.filt(f, x)
    assert sr.rel_err(clean, ref) <= C_BOUND * sr.rel_err(ser, ref)
    i = seglen + 5
    x[i, 1] = np.nan
    y = d.filt(f, x)
    mask, _ = sr.sos_filt(tb, g, x, dt)
    assert np.array_equal(y[:i], clean[:i])
    assert np.array_equal(np.isfinite(y), np.isfinite(mask))
    assert np.array_equal(y[:, 0], clean[:, 0])


@pytest.fixture(scope="module")
def refs():
    """The restatements of one filter per real type, computed once: butter5_02 on 3 tiles + 5 samples, two columns."""
    out = {}
    tb, g = sc.table("butter5_02")
    for dt in (np.float32, np.float64):
        x = sc.signal(3 * 1024 + 5, 2, dt)
        ref, st_ref = sr.sos_filt(tb, g, x, np.longdouble)
        ser, st_ser = sr.sos_filt(tb, g, x, dt)
        out[np.dtype(dt).name] = (x, ref, sr.rel_err(ser, ref), st_ref, sr.rel_err(st_ser, st_ref))
    return out


def _sos(d, name="butter5_02", coef_dtype=np.float64):
    tb, g = sc.table(name)
    return d.SecondOrderSections([d.Biquad(*(np.dtype(coef_dtype).type(v) for v in row)) for row in tb], np.dtype(coef_dtype).type(g))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_filt_and_filt_bang(d, refs, dt):
    import torch
    x, ref, e_serial, _, _ = refs[np.dtype(dt).name]
    f = _sos(d, coef_dtype=dt)
    y = d.filt(f, x)
    assert isinstance(y, np.ndarray) and y.dtype == np.dtype(dt) and y.shape == x.shape
    assert sr.rel_err(y, ref) <= C_BOUND * e_serial
    assert np.array_equal(d.filt(f, x), y)                                     # the same call twice: identical bits
    xt = torch.from_numpy(x).cuda()
    yt = d.filt(f, xt)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and np.array_equal(yt.cpu().numpy(), y)
    assert np.array_equal(xt.cpu().numpy(), x)                                 # the caller's tensor is not filtered in place
    v = torch.from_numpy(np.ascontiguousarray(x[:, 0])).cuda()                 # a device vector already of the working type: its memory is the column
    assert np.array_equal(d.filt(f, v).cpu().numpy(), y[:, 0]) and np.array_equal(v.cpu().numpy(), x[:, 0])
    out = np.empty_like(x)
    assert d.filt_(out, f, x) is out and np.array_equal(out, y)
    outt = torch.empty_like(xt)
    assert d.filt_(outt, f, xt) is outt and np.array_equal(outt.cpu().numpy(), y)
    with pytest.raises(d.DimensionMismatch, match="out size must match x"):
        d.filt_(np.empty((5, 2), dt), f, x)
    # a ZeroPoleGain is converted first; a PolynomialRatio goes to filt(b, a, x), which still refuses a vector a
    z, p, k = sc.ZPK_BUTTER5
    yz = d.filt(d.ZeroPoleGain(np.array(z), np.array(p), k), x.astype(np.float64))
    assert sr.rel_err(yz, ref) <= 1e-9
    with pytest.raises(d.UnsupportedError):
        d.filt(d.PolynomialRatio(d.coefb(f), d.coefa(f)), x)
    assert np.allclose(d.filt(d.PolynomialRatio([1.0, 2.0], [2.0]), x), d.filt(np.array([0.5, 1.0]), 1.0, x))


def test_promotion_nd_and_empty(d, refs):
    x, ref, e_serial, _, _ = refs["float32"]
    f64 = _sos(d)
    y = d.filt(f64, x)                                                         # Float64 coefficients on a Float32 signal: Float64, as in the reference
    assert y.dtype == np.float64
    ref64, _ = sr.sos_filt(*sc.table("butter5_02"), x.astype(np.float64), np.longdouble)
    ser64, _ = sr.sos_filt(*sc.table("butter5_02"), x.astype(np.float64), np.float64)
    assert sr.rel_err(y, ref64) <= C_BOUND * sr.rel_err(ser64, ref64)
    q = d.Biquad(*(np.float32(v) for v in sc.table("butter2_02")[0][0]))
    xi = sc.small_integers(100, 1, np.int32)
    assert d.filt(q, xi).dtype == np.float32                                   # an integer signal does not widen a Float32 filter
    xc = sc.signal(300, 2, np.complex64)
    yc = d.filt(q, xc)
    row = np.array([sc.table("butter2_02")[0][0]], np.float32)                # the coefficients as the Float32 Biquad holds them
    refc, _ = sr.sos_filt(row, 1.0, xc, np.longdouble, has_gain=False)
    serc, _ = sr.sos_filt(row, 1.0, xc, np.float32, has_gain=False)
    assert yc.dtype == np.complex64 and sr.rel_err(yc, refc) <= C_BOUND * sr.rel_err(serc, refc)
    xn = sc.signal(500, 6, np.float64).reshape(500, 2, 3)                      # N-d: the columns are everything after axis 0
    yn = d.filt(f64, xn)
    assert yn.shape == xn.shape and np.array_equal(yn.reshape(500, 6), d.filt(f64, xn.reshape(500, 6)))
    for shape in ((0,), (0, 3), (5, 0)):
        e = d.filt(f64, np.zeros(shape, np.float32))
        assert e.shape == shape and e.dtype == np.float64
    assert d.filtfilt(f64, np.zeros((0, 2))).shape == (0, 2)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_df2tfilter_carries_the_state(d, refs, dt):
    x, ref, e_serial, st_ref, e_state = refs[np.dtype(dt).name]
    n = len(x)
    f = _sos(d, coef_dtype=dt)
    K = len(f.biquads)
    _, _, tile, P, _ = d.sos_geometry(K, dt, 1, 1)
    for split in (1, P - 1, P, tile + 1, n - 1):
        sf = d.DF2TFilter(f, coldims=(2,))
        assert tuple(sf.state.shape) == (2, K, 2) and sf.state.cpu().numpy().dtype == np.dtype(dt)
        y = np.concatenate([d.filt(sf, x[:split]), sf.filt(x[split:])])
        assert sr.rel_err(y, ref) <= C_BOUND * e_serial, split
        assert sr.rel_err(sf.state.cpu().numpy(), st_ref) <= C_BOUND * max(e_state, float(np.finfo(dt).eps)), split
    sf = d.DF2TFilter(f, coldims=(2,))
    with pytest.raises(d.ArgumentError, match="state size must match x"):
        sf.filt(x[:, 0])
    out = np.empty((10, 2), dt)
    assert d.filt_(out, sf, x[:10]) is out
    # a Biquad: state (2, coldims...); a wider signal widens the state for good
    q = d.Biquad(*(np.float32(v) for v in sc.table("butter2_02")[0][0]))
    sq = d.DF2TFilter(q, coldims=(2,))
    assert tuple(sq.state.shape) == (2, 2) and sq.state.cpu().numpy().dtype == np.float32
    x32, x64 = x.astype(np.float32), x.astype(np.float64)
    y1 = sq.filt(x32[:100])
    assert y1.dtype == np.float32
    y2 = sq.filt(x64[100:200])
    assert y2.dtype == np.float64 and sq.state.cpu().numpy().dtype == np.float64
    row = np.array([sc.table("butter2_02")[0][0]], np.float32)                # the coefficients as the Float32 Biquad holds them
    ref1, str1 = sr.sos_filt(row, 1.0, x32[:100], np.longdouble, has_gain=False)
    ser1, st1 = sr.sos_filt(row, 1.0, x32[:100], np.float32, has_gain=False)
    assert sr.rel_err(y1, ref1) <= C_BOUND * sr.rel_err(ser1, ref1)
    # the second piece starts from the Float32 state of the first, widened: compare with the restatement started from ITS Float32 state, in Float32 terms
    want2, _ = sr.sos_filt(row, 1.0, x64[100:200], np.float64, state=st1.astype(np.float64), has_gain=False)
    assert sr.rel_err(y2, want2) <= C_BOUND * max(sr.rel_err(st1, str1), float(np.finfo(np.float32).eps))
    assert d.DF2TFilter(f, dtype=np.float64).state.cpu().numpy().dtype == np.float64
    # the FIR form is untouched
    fir = d.DF2TFilter(np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(fir.filt(np.array([1.0, 0.0, 0.0, 0.0])), [1.0, 2.0, 3.0, 0.0])


@pytest.mark.parametrize("name", ["butter2_02", "butter5_02", "butter8_02"])
def test_filtfilt(d, name):
    import torch
    tb, g = sc.table(name)
    K = len(tb)
    f = _sos(d, name)
    for n, ncols in ((2, 1), (6 * K, 1), (6 * K + 1, 1), (300, 1), (300, 2)):
        x = sc.signal(n, ncols, np.float64, salt=n)
        ref = sr.sos_filtfilt(tb, g, x, np.longdouble)
        e_serial = max(sr.rel_err(sr.sos_filtfilt(tb, g, x, np.float64), ref), float(np.finfo(np.float64).eps))
        y = d.filtfilt(f, x)
        assert y.shape == x.shape and y.dtype == np.float64
        assert sr.rel_err(y, ref) <= C_BOUND * e_serial, n
        if n == 300:
            yt = d.filtfilt(f, torch.from_numpy(x).cuda())
            assert yt.is_cuda and np.array_equal(yt.cpu().numpy(), y)
            z, p, k = d.ZeroPoleGain(f).z, d.ZeroPoleGain(f).p, d.ZeroPoleGain(f).k
            assert np.allclose(d.filtfilt(d.ZeroPoleGain(z, p, k), x), y, rtol=1e-6, atol=1e-9)
    q = d.Biquad(*tb[0])
    x = sc.signal(300, 1, np.float64)
    assert np.array_equal(d.filtfilt(q, x), d.filtfilt(d.SecondOrderSections([q], 1), x))       # a Biquad goes through its one-section cascade
    with pytest.raises(d.UnsupportedError):
        d.filtfilt(d.PolynomialRatio(d.coefb(f), d.coefa(f)), x)                                # filtfilt(b, a, x) with a vector a: as before


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_a_nan_sample(d, dt):
    _, _, tile, P, _ = d.sos_geometry(1, dt, 1, 1)
    n, i = 2 * tile + 3, tile + 5
    for f, rows, g, has_gain in ((_sos(d, coef_dtype=dt), *sc.table("butter5_02"), True), (d.Biquad(*sc.FIR_ONLY), [sc.FIR_ONLY], 1.0, False)):
        x = sc.signal(n, 3, dt)
        clean = d.filt(f, x)
        x[i, 1] = np.nan
        y = d.filt(f, x)
        ref, _ = sr.sos_filt(rows, g, x, dt, has_gain=has_gain)
        assert np.array_equal(y[:i], clean[:i])                                 # before the sample: as without it
        assert np.array_equal(np.isfinite(y), np.isfinite(ref))                 # from it on: the restatement's mask
        assert np.array_equal(y[:, [0, 2]], clean[:, [0, 2]])                   # the other columns are untouched
