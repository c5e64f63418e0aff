"""GPU tests of mdsp_welch_w64d_asm (csrc/welch_w64d_asm.s, Welch variant 44: variant 43 with folded twiddles, tools/gen_welch_asm_d.py): against the
Float64 oracle, against variant 43 (the same frames and accumulators; only the rounding of the twiddled butterflies differs), deterministic, and the
kernel a plain Welch call of a long Float32 stream takes at nfft 4096."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL32 = 5e-6


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _welch(d, s, variant, window=None):
    from dsp_jl_amd import _lib
    _lib.set_tunable("MDSP_WELCH_VARIANT", None if variant is None else str(variant))
    try:
        cfg = d.WelchConfig(s.shape[0], np.float32, n=4096, noverlap=2048, window=window or d.hanning, engine=d.ENGINE_FUSED)
        return d.welch_pgram(s, cfg).power
    finally:
        _lib.set_tunable("MDSP_WELCH_VARIANT", None)


def test_w64d_vs_oracle_and_w64c(d):
    from oracle import periodograms as opg, windows as ow
    rng = np.random.default_rng(4404)
    for length in (4096, 8192, 10240, 100_000, 4096 * 700 + 2048, (1 << 23) + 4097, (1 << 23) + 4096 * 129):
        s = (rng.standard_normal(length) + 0.5 * np.sin(2 * np.pi * 0.1234 * np.arange(length))).astype(np.float32)
        got = _welch(d, s, 44)
        assert np.array_equal(got, _welch(d, s, 44)), length                       # deterministic
        old = _welch(d, s, 43)
        if length >= 100_000:
            assert not np.array_equal(got, old), length                             # the two kernels did run: their roundings differ
        assert relerr(got, old.astype(np.float64)) < 1e-6, (length, relerr(got, old.astype(np.float64)))
        if length <= 4096 * 700 + 2048:
            ref = opg.welch_pgram(s, 4096, 2048, window=ow.hanning, dtype=np.float64).power
            assert relerr(got, ref) < TOL32, (length, relerr(got, ref))


def test_w64d_is_the_default_for_long_streams(d):
    from oracle import periodograms as opg, windows as ow
    rng = np.random.default_rng(4405)
    L = (1 << 23) + 4096 * 3 + 2048          # odd frame count: the last frame goes through welch_half3_kernel
    s = (rng.standard_normal(L) + 0.25 * np.sin(2 * np.pi * 0.05 * np.arange(L))).astype(np.float32)
    dflt = _welch(d, s, None)
    assert np.array_equal(dflt, _welch(d, s, 44))
    assert relerr(dflt, opg.welch_pgram(s, 4096, 2048, window=ow.hanning, dtype=np.float64).power) < TOL32


def test_w64d_several_channels(d):
    rng = np.random.default_rng(4406)
    L = (1 << 23) + 4096
    S = rng.standard_normal((L, 3)).astype(np.float32)
    P = _welch(d, S, 44, window=d.hamming)
    for c in range(3):
        one = _welch(d, S[:, c].copy(), 44, window=d.hamming)
        assert relerr(P[:, c], one.astype(np.float64)) < 1e-6, c
    assert relerr(P, _welch(d, S, 43, window=d.hamming).astype(np.float64)) < 1e-6


def test_w64_asm_kernels_over_several_flushes(d):
    """Every wave of the chip runs 129 units of one channel (a stream of 2^30 + 2^21 samples on a 256-CU part), so each writes TWO partial rows: the
    Float32 run sums are flushed after 128 units and again at the end.  Variants 44 and 43 against welch_half3_kernel (variant 30)."""
    import torch
    from dsp_jl_amd import _lib
    lib = _lib.lib()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    units = cu * 8 * 128 + cu * 4                      # half of the 8 cu waves get a 129th unit, at most ceil(units / (8 cu)) = 129 per wave
    n = 4096 * units + 2048
    g = torch.Generator(device="cuda")
    g.manual_seed(4407)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    psd = torch.empty(2049, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for v in (44, 43, 30):
        _lib.set_tunable("MDSP_WELCH_VARIANT", str(v))
        try:
            cfg = d.WelchConfig(n, np.float32, n=4096, noverlap=2048, window=d.hanning, engine=d.ENGINE_FUSED)
        finally:
            _lib.set_tunable("MDSP_WELCH_VARIANT", None)
        _lib.check(lib.mdsp_welch_exec(cfg._h, x.data_ptr(), n, 1, n, psd.data_ptr(), 2049, st))
        torch.cuda.synchronize()
        out[v] = psd.cpu().numpy().astype(np.float64)
    del x
    assert np.all(np.isfinite(out[44])) and not np.array_equal(out[44], out[43])
    assert relerr(out[44], out[30]) < 1e-6, relerr(out[44], out[30])
    assert relerr(out[43], out[30]) < 1e-6, relerr(out[43], out[30])
