"""CPU checks of tests/mt_cross_ref.py, the long-double reference of the multitaper cross-spectra sweep (tests/test_gpu_mt_cross.py):

  * it agrees with oracle.multitaper (mt_cross_power_spectra, coherence_from_cs) to 1e-13 norm-wise on random shapes -- odd and even nfft, a frequency
    band on and off, demean on and off;
  * the bounds the sweep applies -- per (taper, channel) column 8 log2(nfft) u max|ref|; per cross-spectral component (ntapers + 8) u absdot + 2 u_min;
    per coherence 6 u |ref|; demean bit for bit -- pass an emulation of the kernels in Float32 and in Float64 (plain numpy, the kernels' order of
    operations) and fail seven subtly wrong ones: the bounds are not vacuous;
  * the case table (mt_cross_ref.MT_CASES) is what guard_cases.spectral_cases and the committed route table make it: a table edit cannot drop a route.

The emulated transform is numpy's Float64 rfft of the product rounded to R, rounded to R again: about one rounding per bin, so the emulation says that a
CORRECT column passes and a wrong one does not; how close the device's own FFT comes to the bar is what the GPU file measures."""
import numpy as np
import pytest

import guard_cases as gc
import mt_cross_ref as mr
from conftest import relerr
from oracle import multitaper as omt

LD = mr.LD
TYPES = [np.float32, np.float64]


# ---- the kernels, emulated in R ------------------------------------------------------------------------------------------------------------------------
def emu_demean(sig, R, defect=None):
    s = np.ascontiguousarray(sig, dtype=R)
    m = (s.astype(np.float64).sum(axis=1) / np.float64(s.shape[1])).astype(R)
    if defect == "neighbour-mean" and s.shape[0] > 1:
        m[1] = m[0]
    return s - m[:, None]


def emu_spectra(sig, tapers, nfft, demean, R, defect=None):
    """x_mt[f, k, c] in complex R: demean_kernel, then per taper the windowed frame (Float64 window, product rounded to R) and its transform."""
    s = emu_demean(sig, R, defect) if demean else np.ascontiguousarray(sig, dtype=R)
    t = tapers[::-1] if defect == "taper-reversed" else tapers
    prod = (t.T[None, :, :] * s.astype(np.float64)[:, None, :]).astype(R)
    X = np.fft.rfft(prod.astype(np.float64), n=nfft, axis=2).transpose(2, 1, 0)
    return np.ascontiguousarray(X).astype(np.complex64 if R == np.float32 else np.complex128)


def emu_cross(x, w, freq_inds, nfft, R, defect=None):
    """cross_spectra_kernel step by step in R: the divisions by R(sqrt 2), a conj(b), the weight rounded to R, the running sums."""
    nout, ntap, nch = x.shape
    fi = np.asarray(freq_inds)
    root2 = R(1.4142135623730951)
    even = nfft % 2 == 0
    if defect == "nyquist-scaled-odd":
        even = True
    if defect == "nyquist-unscaled-even":
        even = False
    edge = ((fi == 0) | (even & (fi == nout - 1)))[:, None]
    out = np.zeros((nch, nch, fi.size), dtype=x.dtype)
    for l in range(nch):
        for m in range(nch):
            ax = np.zeros(fi.size, dtype=R)
            ay = np.zeros(fi.size, dtype=R)
            a, b = x[fi][:, :, l], x[fi][:, :, m]                                   # (nfi, ntapers)
            a_x, a_y = np.where(edge, a.real / root2, a.real), np.where(edge, a.imag / root2, a.imag)
            b_x, b_y = np.where(edge, b.real / root2, b.real), np.where(edge, b.imag / root2, b.imag)
            if defect == "conj-wrong-operand":
                a_y, b_y = -a_y, -b_y
            for k in range(ntap):
                wk = R(w[(k + 1) % ntap if defect == "weight-off-by-one" else k])
                px = a_x[:, k] * b_x[:, k] + a_y[:, k] * b_y[:, k]
                py = a_y[:, k] * b_x[:, k] - a_x[:, k] * b_y[:, k]
                ax = ax + wk * px
                ay = ay + wk * py
            out[l, m].real, out[l, m].imag = ax, ay
    return out


def emu_coherence(cs, R, defect=None):
    nch, _, nf = cs.shape
    out = np.empty((nch, nch, nf), dtype=R)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c1 in range(nch):
            for c2 in range(nch):
                if c1 == c2:
                    out[c1, c2] = 1
                    continue
                hi, lo = max(c1, c2), min(c1, c2)
                f = np.arange(nf)
                if defect == "mirror-wrong-frequency" and c1 < c2:
                    f = (f + 1) % nf
                v, d1, d2 = cs[hi, lo, f], cs[hi, hi, f], cs[lo, lo, f]
                out[c1, c2] = np.sqrt(v.real * v.real + v.imag * v.imag) / np.sqrt(d1.real * d2.real - d1.imag * d2.imag)
    return out


def _case(R, nfft, nch=3, ntap=3, seed=0):
    rng = np.random.default_rng(7700 + seed + nfft)
    n = nfft - nfft // 4 - 1
    tapers, r = mr.random_tapers(rng, n, ntap)
    sig = mr.dyadic_signal(rng, nch, n, R)
    nout = nfft // 2 + 1
    fi = np.concatenate([[nout - 1, 0], rng.permutation(np.arange(1, nout - 1))[:5]])
    return sig, tapers, 2.0 / r, fi


def _verdicts(R, nfft, defect):
    """(column excess, demean bits equal, cross excess, coherence excess) of one emulation against the reference's bounds."""
    sig, tapers, w, fi = _case(R, nfft)
    x = emu_spectra(sig, tapers, nfft, True, R, defect)
    col, _ = mr.column_excess(x, mr.tapered_spectra(sig, tapers, nfft, True, R), nfft, R)
    bits = np.array_equal(emu_demean(sig, R, defect), mr.demean(sig, R))
    good = emu_spectra(sig, tapers, nfft, True, R)                 # the later stages start from a correct x_mt, as the GPU tests give them synthetic input
    ref, absdot = mr.cross_spectra(good, w, fi, nfft)
    cross, _ = mr.cross_excess(emu_cross(good, w, fi, nfft, R, defect), ref, absdot, tapers.shape[1], R)
    cs = mr.hermitian_input(ref, R)
    coh = mr.coherence_excess(emu_coherence(cs, R, defect), mr.coherence(cs), R)
    return col, bits, cross, coh


# ---- the reference against the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_reference_equals_the_oracle(seed):
    rng = np.random.default_rng(5100 + seed)
    n = int(rng.integers(8, 200))
    nfft = n + int(rng.integers(0, 50))
    nfft += (nfft + seed) % 2                                       # odd on odd seeds, even on even ones
    nch, ntap = int(rng.integers(1, 5)), int(rng.integers(1, 6))
    demean, band = bool(seed & 2), bool(seed & 4)
    fs = 100.0
    tapers, _ = mr.random_tapers(rng, n, ntap)
    weights = rng.uniform(0.5, 1.5, ntap)
    sig = rng.standard_normal((nch, n)) + 3.0
    mc = omt.MTConfig(np.float64, n, fs=fs, nfft=nfft, window=tapers, ntapers=ntap, taper_weights=weights)
    nout = nfft // 2 + 1
    lo, hi = sorted(int(v) for v in rng.choice(nout, 2, replace=False))
    cfg = omt.MTCrossSpectraConfig(nch, mc, demean=demean, freq_range=(mc.freq[lo], mc.freq[hi]) if band else None)
    want, _ = omt.mt_cross_power_spectra(sig, cfg)
    x = mr.tapered_spectra(sig, tapers, nfft, demean, np.float64)
    cs, absdot = mr.cross_spectra(x, 2.0 / mc.r, cfg.freq_inds, nfft)
    assert cs.shape == want.shape == (nch, nch, len(cfg.freq_inds))
    assert len(cfg.freq_inds) == (hi - lo - 1 if band else nout)          # the ends of the band are open
    if cs.size:
        assert relerr(cs.astype(np.complex128), want) < 1e-13, (n, nfft, nch, ntap, demean, band)
        assert np.all(absdot.real >= np.abs(cs.real) * (1 - 1e-15)) and np.all(absdot.imag >= np.abs(cs.imag) * (1 - 1e-15))
        if nch > 1:
            assert relerr(mr.coherence(want).astype(np.float64), omt.coherence_from_cs(want)) < 1e-13
            assert relerr(mr.coherence(cs).astype(np.float64), omt.coherence_from_cs(want)) < 1e-12


def test_reference_scales_the_last_row_on_even_nfft_only():
    x = np.ones((5, 1, 1), dtype=complex)
    for nfft, last in ((8, 0.5), (9, 1.0)):
        cs, _ = mr.cross_spectra(x, [1.0], np.arange(5), nfft)
        assert np.allclose(cs[0, 0].real.astype(float), [0.5, 1, 1, 1, last], rtol=1e-15, atol=0)


def test_reference_coherence_diagonal_mirror_and_nan():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 3, 4)) + 1j * rng.standard_normal((4, 3, 4))
    x[:, :, 2] = 0
    cs, _ = mr.cross_spectra(x, [1.0, 2.0, 0.5], np.arange(4), 7)
    c = mr.coherence(cs)
    assert np.all(c[np.arange(4), np.arange(4)] == 1)
    assert np.array_equal(np.isnan(c), np.isnan(c.transpose(1, 0, 2)))
    nan = np.zeros((4, 4), dtype=bool)
    nan[2, :] = nan[:, 2] = True
    nan[2, 2] = False
    assert np.array_equal(np.isnan(c), np.broadcast_to(nan[:, :, None], c.shape))
    ok = ~np.isnan(c)
    assert np.array_equal(c[ok], c.transpose(1, 0, 2)[ok]) and np.all(c[ok] <= 1 + 1e-18)


@pytest.mark.parametrize("R", TYPES)
def test_demean_reference_is_the_exact_sum_on_the_dyadic_grid(R):
    from fractions import Fraction
    rng = np.random.default_rng(11)
    s = mr.dyadic_signal(rng, 2, 301, R)
    got = mr.demean(s, R)
    for c in range(2):
        exact = sum(Fraction(float(v)) for v in s[c])
        assert Fraction(float(s[c].astype(np.float64).sum())) == exact                  # Float64 holds the sum exactly ...
        assert Fraction(float(np.sum(s[c, ::-1].astype(np.float64)))) == exact          # ... in any order
        m = R(float(exact) / 301) if float(exact) == exact else None
        assert m is not None
        want = np.array([R(v) - m for v in s[c]], dtype=R)
        assert np.array_equal(got[c], want)
        # one rounding: the stored value is the R nearest to the exact difference
        for v, g in zip(s[c, :16], got[c, :16]):
            d = Fraction(float(v)) - Fraction(float(m))
            assert abs(Fraction(float(g)) - d) <= abs(Fraction(float(np.nextafter(g, R(np.inf)))) - d)
            assert abs(Fraction(float(g)) - d) <= abs(Fraction(float(np.nextafter(g, R(-np.inf)))) - d)


# ---- the bounds are not vacuous -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [64, 75])
@pytest.mark.parametrize("R", TYPES)
def test_bounds_pass_a_correct_emulation(R, nfft):
    col, bits, cross, coh = _verdicts(R, nfft, None)
    assert col < 1.0 and bits and cross <= 1.0 and coh <= 1.0, (col, bits, cross, coh)


@pytest.mark.parametrize("R", TYPES)
@pytest.mark.parametrize("ntap", [1, 3, 7])
@pytest.mark.parametrize("nfft", [8, 9, 256, 75])
def test_cross_bound_passes_every_taper_count_and_the_edge_rows(R, ntap, nfft):
    rng = np.random.default_rng(ntap + nfft)
    nout = nfft // 2 + 1
    cdt = np.complex64 if R == np.float32 else np.complex128
    x = (rng.standard_normal((nout, ntap, 4)) + 1j * rng.standard_normal((nout, ntap, 4))).astype(cdt)
    _, r = mr.random_tapers(rng, 8, ntap)
    for fi in (np.arange(nout), [0], [nout - 1]):
        ref, absdot = mr.cross_spectra(x, 2.0 / r, fi, nfft)
        worst, ratio = mr.cross_excess(emu_cross(x, 2.0 / r, fi, nfft, R), ref, absdot, ntap, R)
        assert worst <= 1.0, (ntap, nfft, worst, ratio)


WRONG = [  # (defect, nfft at which it shows, the check that must catch it)
    ("nyquist-scaled-odd", 75, "cross"),
    ("nyquist-unscaled-even", 64, "cross"),
    ("conj-wrong-operand", 64, "cross"),
    ("weight-off-by-one", 75, "cross"),
    ("taper-reversed", 64, "column"),
    ("mirror-wrong-frequency", 75, "coherence"),
    ("neighbour-mean", 64, "column+demean"),
]


@pytest.mark.parametrize("R", TYPES)
@pytest.mark.parametrize("defect,nfft,caught_by", WRONG)
def test_bounds_fail_each_wrong_emulation(R, defect, nfft, caught_by):
    col, bits, cross, coh = _verdicts(R, nfft, defect)
    if caught_by == "cross":
        assert cross > 1.0 and col < 1.0 and coh <= 1.0, (col, cross, coh)
    elif caught_by == "column":
        assert col >= 1.0 and cross <= 1.0, (col, cross)
    elif caught_by == "coherence":
        assert coh > 1.0 and cross <= 1.0 and col < 1.0, (col, cross, coh)
    else:
        assert col >= 1.0 and not bits, (col, bits)


@pytest.mark.parametrize("R", TYPES)
def test_scaling_defects_are_invisible_on_the_other_parity(R):
    # what the old single even size could never see: the odd-size defect does nothing at an even size and the other way round -- both parities are needed
    assert _verdicts(R, 64, "nyquist-scaled-odd")[2] <= 1.0
    assert _verdicts(R, 75, "nyquist-unscaled-even")[2] <= 1.0


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_case_table_is_the_committed_route_table(dtype):
    import spectral_route_cases as src
    table = src.expected_default()
    cases = mr.MT_CASES[dtype]
    assert len(set(cases)) == len(cases)
    auto_at = dict(zip(src.SIZES, table[(gc.KIND_STFT, dtype, gc.AUTO)][0]))
    rocfft_at = dict(zip(src.SIZES, table[(gc.KIND_STFT, dtype, gc.ROCFFT)][0]))
    # every size takes the route the case names ('-' would be a size without a plan: a failure here, never a skip on the device)
    for engine, nfft, route in cases:
        assert route != "-" and {gc.AUTO: auto_at, gc.ROCFFT: rocfft_at}[engine][nfft] == route, (engine, nfft, route)
    # under AUTO: the smallest nfft >= 8 of every route -- what the guard-band suite takes from the same table, the first power-of-two size only
    first = {}
    for e, n, c in gc.spectral_cases(gc.KIND_STFT, dtype):
        if e == gc.AUTO:
            first.setdefault(c, n)
    smallest = {(gc.AUTO, n, c) for c, n in first.items()}
    assert smallest <= set(cases), smallest - set(cases)
    # and the smallest odd size of every route that has one the long-double DFT reaches
    odd = {}
    for n, c in zip(src.SIZES, table[(gc.KIND_STFT, dtype, gc.AUTO)][0]):
        if n >= 8 and n % 2 == 1 and c != "-":
            odd.setdefault(c, n)
    smallest_odd = {(gc.AUTO, n, c) for c, n in odd.items() if n <= mr.DFT_MAX}
    assert smallest_odd <= set(cases), smallest_odd - set(cases)
    assert set(cases) == smallest | smallest_odd | {(gc.ROCFFT, gc.ROCFFT_NFFT, "0")}
    # the sizes above DFT_MAX are the multi-pass ones, the only ones without a long-double claim
    assert {n for e, n, c in cases if n > mr.DFT_MAX} == {n for e, n, c in cases if c == mr.MULTIPASS_ROUTE}


@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_case_table_is_what_the_library_answers(dtype):
    """mdsp_spectral_route_for on the built library: host arithmetic, no device."""
    import spectral_route_cases as src
    from dsp_jl_amd import _lib
    for engine, nfft, route in mr.MT_CASES[dtype]:
        assert src.encode(_lib.lib(), gc.KIND_STFT, dtype, engine, [nfft])[0] == route, (engine, nfft)
