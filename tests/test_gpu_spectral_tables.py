"""A spectral plan's root and window tables are built at its creation (csrc/spectral_tables.h; DESIGN.md, spectral section): whatever stream the first
call runs on, and whether or not it has any frame, finds them complete.  One case per Welch route 1, 2, 3, 4, 6, 7, 8, 9 and element type that reaches it -- nfft 256 on
the power-of-two route, elsewhere the smallest size of tests/ct_schedule_cases.py's route table -- 3 frames at 50 % overlap under ct.window(n), 2 channels; and one
Float32 stream of nfft 4096 just long enough for the hand-allocated kernel (eight units per CU, as tests/test_gpu_welch_w64d.py sizes it), whose prepared block
is such a table too.  Every comparison is bit for bit.

    a. first use on another stream: a fresh WelchConfig makes its first call on a side stream (which waited for the input), its second on the default stream
       behind an event and no host synchronisation; both equal a second fresh config run on the default stream alone.
    b. empty first slice: reset, accumulate a slice shorter than n (no frame), accumulate the signal, finalize: equals the one-shot result.
    c. multitaper: mt_pgram of a complex signal at the smallest size on the single-workgroup columns, 3 tapers, twice on one plan: bit-identical, and within
       tests/test_gpu_gx.py's bound of the oracle -- the sites that convert the window of each launch (the taper changes between passes) still do.

Case a states the contract; it is not a regression test.  Before tables were built at creation, some routes filled them on the stream of the first call and a call
on another stream could read them too early -- a race that depends on timing, so this test could pass there as well."""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr

import ct_schedule_cases as ct

pytestmark = pytest.mark.gpu

ROUTES = (1, 2, 3, 4, 6, 7, 8, 9)
TOL32 = 5e-6


def _nfft(route, dtype):
    """the smallest size on the route (nfft 256 on the power-of-two route) -- from 3 points: ct.window(2) is all zeros, which no WelchConfig accepts"""
    if route == 1:
        return 256
    return next((c.nfft for c in ct.on_route(ct.WELCH, dtype, route) if c.nfft >= 3), None)


CASES = [pytest.param(route, dtype, _nfft(route, dtype), id=f"route{route}-{ct.NP_DTYPES[dtype].name}-{_nfft(route, dtype)}")
         for route in ROUTES for dtype in ct.DTYPES if _nfft(route, dtype)]


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _route(kind, dtype, nfft):
    from dsp_jl_amd import _lib
    eng, route, r0 = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().mdsp_spectral_route_for(kind, dtype, nfft, ct.AUTO, C.byref(eng), C.byref(route), C.byref(r0)))
    return route.value


def _check_plan(d, x, n, make_config):
    """cases a and b for the device columns x (length, channels); make_config() gives a fresh WelchConfig of n-sample frames"""
    import torch
    uploaded = torch.cuda.Event()
    uploaded.record()
    # a.
    side = torch.cuda.Stream()
    wc = make_config()
    with torch.cuda.stream(side):
        side.wait_event(uploaded)
        first = d.welch_pgram(x, wc).power
        done = torch.cuda.Event()
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    second = d.welch_pgram(x, wc).power
    ref = d.welch_pgram(x, make_config()).power
    # b.
    cols = x.t().contiguous()
    wb = make_config()
    wb.reset()
    wb.accumulate(cols[:, : n - 1].contiguous())
    assert wb.frames_accumulated() == 0
    wb.accumulate(cols)
    sliced = wb.finalize(nch=cols.shape[0]).t()
    ref = ref.cpu().numpy()
    assert ref.shape == (wc.nout, x.shape[1]) and np.all(np.isfinite(ref)) and np.all(ref.max(axis=0) > 0)
    assert np.array_equal(first.cpu().numpy(), ref), "first call, on the side stream"
    assert np.array_equal(second.cpu().numpy(), ref), "second call, on the default stream"
    assert np.array_equal(sliced.cpu().numpy(), ref), "after an empty first slice"


@pytest.mark.parametrize("route,dtype,nfft", CASES)
def test_tables_exist_before_the_first_call(d, route, dtype, nfft):
    import torch
    assert _route(ct.WELCH, dtype, nfft) == route
    dt = ct.NP_DTYPES[dtype]
    length = 2 * (nfft - nfft // 2) + nfft                      # 3 frames of nfft samples at 50 % overlap
    s = np.stack([ct.signal((route, dtype, c), length, dt) for c in range(2)], axis=1)
    x = torch.from_numpy(s).to("cuda")

    def make_config():
        wc = d.WelchConfig(length, dt, n=nfft, noverlap=nfft // 2, nfft=nfft, window=ct.window(nfft), fs=2.5)
        assert wc.engine == d.ENGINE_FUSED
        return wc

    _check_plan(d, x, nfft, make_config)


def test_prepared_block_of_the_nfft_4096_kernel(d):
    import torch
    assert _route(ct.WELCH, ct.F32, 4096) == 1
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    K = 16 * cu                            # K / 2 = 8 units per CU: the hand-allocated kernel (welch.hip welch_launch_n)
    length = (K - 1) * 2048 + 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(4096)
    x = torch.randn((length, 1), generator=g, device="cuda", dtype=torch.float32)
    _check_plan(d, x, 4096, lambda: d.WelchConfig(length, np.float32, n=4096, noverlap=2048, window=ct.window(4096), engine=d.ENGINE_FUSED))


def test_multitaper_converts_the_window_of_each_launch(d):
    from oracle import multitaper as omt
    case = ct.direct(ct.STFT, ct.C32)[0]
    n = case.nfft
    assert _route(ct.STFT, ct.C32, n) == ct.ROUTE_CTBIG_COLS
    x = ct.signal((5, ct.C32), n, np.complex64)
    cfg = d.MTConfig(np.complex64, n, nfft=n, nw=2, ntapers=3, fs=2.0)
    got = d.mt_pgram(x, cfg)
    assert np.array_equal(d.mt_pgram(x, cfg).power, got.power)
    ref_power, ref_freq = omt.mt_pgram(x.astype(np.complex128), nw=2, ntapers=3, fs=2.0, nfft=n)
    assert np.array_equal(got.freq, ref_freq)
    assert relerr(got.power, ref_power) < TOL32, relerr(got.power, ref_power)
