"""The two tables every Welch / STFT plan builds at its creation (dsp.jl_amd/csrc/spectral_tables.h, host part), compiled with g++
(tests/cpu_harness/spectral_tables.cpp) and compared with numpy: the window in the working precision and the table of forward roots of unity."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [pytest.param("f32", np.float32, id="float32"), pytest.param("f64", np.float64, id="float64")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("spectral_tables") / "spectral_tables")
    r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpu_harness", "spectral_tables.cpp"), "-o", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def _values(exe, R, *args):
    """the program's output: one value per line, the hexadecimal of its bits"""
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    bits = np.array([int(line, 16) for line in r.stdout.split()], dtype=np.uint32 if R is np.float32 else np.uint64)
    return bits.view(R)


@pytest.mark.parametrize("prec,R", PRECISIONS)
def test_working_window(exe, prec, R):
    nfft = 4096
    for n in (nfft, nfft - 7, 1):
        win = 1.0 / (np.arange(n) + 3.0)                       # the harness's window: one IEEE division per value
        for have_window in (1, 0):
            got = _values(exe, R, "window", prec, n, nfft, have_window)
            assert got.dtype == R and got.shape == (nfft,)
            want = win.astype(R) if have_window else np.ones(n, dtype=R)
            assert np.array_equal(got[:n], want), (n, have_window)
            assert np.all(got[n:] == 0) and not np.any(np.signbit(got[n:])), (n, have_window)      # exactly zero behind the window
    assert not np.array_equal(win.astype(np.float32).astype(np.float64), win)          # the cast to Float32 did round


@pytest.mark.parametrize("prec,R", PRECISIONS)
def test_root_table(exe, prec, R):
    """Every entry within 1 ulp of R of exp(-2 pi i k / n) evaluated in longdouble.  That reference has an error of its own: the angle 2 pi k / n < 2 pi is the
    result of three longdouble roundings (pi, the product, the quotient), each at most 2^-64 relative, so it is off by at most 3 * 2^-64 * 2 pi < 2^-59, and cos
    and sin move by no more than their argument does.  The entries that are exactly zero (k = n / 4, n / 2 ...) are therefore allowed that much, absolute;
    everywhere else it vanishes against the ulp."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "the reference needs a longdouble wider than Float64"
    pi = 4 * np.arctan(ld(1))
    for n in (7, 4096, 12500):
        got = _values(exe, R, "roots", prec, n)
        assert got.dtype == R and got.shape == (2 * n,)
        re, im = got[0::2], got[1::2]
        assert re[0] == 1 and im[0] == 0
        ang = -2 * pi * np.arange(n, dtype=ld) / ld(n)
        for part, ref in ((re, np.cos(ang)), (im, np.sin(ang))):
            ulp = np.spacing(np.abs(ref).astype(R)).astype(ld)
            err = np.abs(part.astype(ld) - ref)
            assert np.all(err <= ulp + ld(2) ** -59), (n, float(np.max(err / ulp)))
