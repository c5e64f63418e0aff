"""GPU tests of mdsp_welch_w64e_asm (csrc/welch_w64e_asm.s, Welch variant 45; tools/gen_welch_asm_e.py).  It is variant 44 with counted load waits: the
same vector instructions on the same values in the same order, so every case holds it to variant 44 BIT FOR BIT -- a load consumed before it arrived
cannot hide in a tolerance.  (The generator's second switch, streaming sample loads, lost its A/B and is not in the library: nothing to run here.)"""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL32 = 5e-6
NFFT, HOP, NOUT = 4096, 2048, 2049
FORMS = (45,)


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


def _plan(d, n, variant):
    from dsp_jl_amd import _lib
    _lib.set_tunable("MDSP_WELCH_VARIANT", None if variant is None else str(variant))
    try:
        return d.WelchConfig(n, np.float32, n=NFFT, noverlap=HOP, window=d.hanning, engine=d.ENGINE_FUSED)
    finally:
        _lib.set_tunable("MDSP_WELCH_VARIANT", None)


def _power(d, torch, x, n, variant, nch=1, ld=None, plan=None):
    """Float32 power (nch, 2049) of the first n samples of each of nch channels, ld floats apart, starting at x's first element; the launch goes to
    torch's current stream, behind whatever torch queued there"""
    from dsp_jl_amd import _lib
    cfg = plan or _plan(d, n, variant)
    psd = torch.full((nch, NOUT), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().mdsp_welch_exec(cfg._h, x.data_ptr(), n, nch, ld or n, psd.data_ptr(), NOUT, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return psd.cpu().numpy()


def _signal(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    x += 0.5 * torch.sin(2 * np.pi * 0.1234 * torch.arange(n, device="cuda", dtype=torch.float32))
    return x


def _oracle(x):
    from oracle import periodograms as opg, windows as ow
    return opg.welch_pgram(x.cpu().numpy(), NFFT, HOP, window=ow.hanning, dtype=np.float64).power


@pytest.mark.parametrize("K", [2, 3, 4, 5, 1400])
def test_frame_counts_bit_for_bit_and_oracle(d, torch, K):
    """K = 2: one unit; 3: and an odd last frame (welch_half3_kernel); 4, 5: two slots; 1400 frames = 4096 * 700 + 2048 samples: 700 units, one per slot of 88 workgroups"""
    n = HOP * (K + 1)
    x = _signal(torch, n, 4500 + K)
    ref = _power(d, torch, x, n, 44)
    assert np.all(np.isfinite(ref))
    for v in FORMS:
        got = _power(d, torch, x, n, v)
        assert np.array_equal(got, ref), (K, v)
        assert np.array_equal(got, _power(d, torch, x, n, v)), (K, v)           # two calls, identical bits
    e = relerr(ref[0], _oracle(x))
    assert e < TOL32, (K, e)


def test_several_units_per_slot_partial_last_runs_and_idle_slots(d, torch):
    """8 cu slots and 3 x 8 cu + 5 units: runs of 4 units, so most slots walk A B A B, one walks a partial run and the rest none"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    units = cu * 8 * 3 + 5
    n = NFFT * units + HOP
    x = _signal(torch, n, 4510)
    ref = _power(d, torch, x, n, 44)
    assert np.all(np.isfinite(ref)) and ref.max() > 0
    for v in FORMS:
        assert np.array_equal(_power(d, torch, x, n, v), ref), v
    assert not np.array_equal(ref, _power(d, torch, x, n, 43))                  # the variant knob did select kernels: 43 rounds differently


def test_three_channels_with_a_leading_dimension(d, torch):
    n, ld = NFFT * 9 + HOP, NFFT * 9 + HOP + 37
    g = torch.Generator(device="cuda")
    g.manual_seed(4511)
    X = torch.randn((3, ld), generator=g, device="cuda", dtype=torch.float32)
    ref = _power(d, torch, X, n, 44, nch=3, ld=ld)
    for v in FORMS:
        got = _power(d, torch, X, n, v, nch=3, ld=ld)
        assert np.array_equal(got, ref), v
    for c in range(3):
        one = _power(d, torch, X[c].contiguous(), n, 45)
        assert np.array_equal(one[0], ref[c]), c
        assert relerr(ref[c], _oracle(X[c, :n])) < TOL32


def test_signal_one_float_off_a_cache_line(d, torch):
    n = NFFT * 21 + HOP
    buf = torch.zeros(n + 64, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 128 == 0
    buf[1:n + 1] = _signal(torch, n, 4512)
    x = buf[1:]
    assert x.data_ptr() % 128 == 4
    ref = _power(d, torch, x, n, 44)
    for v in FORMS:
        assert np.array_equal(_power(d, torch, x, n, v), ref), v
    aligned = buf[1:n + 1].clone()
    assert np.array_equal(_power(d, torch, aligned, n, 45), ref)
    assert relerr(ref[0], _oracle(aligned)) < TOL32


def test_floats_behind_the_end_are_never_used(d, torch):
    """a wave loads the unit after its last one through an empty descriptor, which returns zeros: NaNs behind the signal must not reach the power"""
    n = NFFT * 11
    buf = torch.zeros(n + 4 * NFFT, dtype=torch.float32, device="cuda")
    buf[:n] = _signal(torch, n, 4513)
    clean = {v: _power(d, torch, buf, n, v) for v in (44,) + FORMS}
    buf[n:] = float("nan")
    for v in (44,) + FORMS:
        got = _power(d, torch, buf, n, v)
        assert np.all(np.isfinite(got)), v
        assert np.array_equal(got, clean[44]), v


def test_kernel_sees_what_a_kernel_on_the_stream_just_wrote(d, torch):
    n = NFFT * 64 + HOP
    x = _signal(torch, n, 4514)
    y = _signal(torch, n, 4515)
    plan = _plan(d, n, 45)
    first = _power(d, torch, x, n, 45, plan=plan)
    x.copy_(y)                                   # a kernel on the same stream overwrites the signal; the launch below is queued right behind it
    second = _power(d, torch, x, n, 45, plan=plan)
    assert not np.array_equal(first, second)
    assert np.array_equal(second, _power(d, torch, y, n, 44))
    x.mul_(-3.0)
    assert np.array_equal(_power(d, torch, x, n, 45, plan=plan), _power(d, torch, y * -3.0, n, 44))


def test_default_route_of_a_long_stream(d, torch):
    n = (1 << 23) + NFFT * 3 + HOP
    x = _signal(torch, n, 4516)
    ref = _power(d, torch, x, n, 44)
    assert np.array_equal(_power(d, torch, x, n, None), ref)
    assert np.array_equal(_power(d, torch, x, n, 45), ref)
    assert not np.array_equal(ref, _power(d, torch, x, n, 43))
