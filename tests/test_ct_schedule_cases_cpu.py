"""The case lists and inputs of tests/ct_schedule_cases.py -- the sweep tests/test_gpu_ct_schedules.py runs over every compile-time spectral schedule --
held to the X-macro size tables of dsp.jl_amd/csrc/ctbig_sizes.h, to the route table of tests/spectral_route_cases.py and to their stated counts, so
that a schedule added to the header without entering the sweep, or a case lost from the generator, fails here.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ct_schedule_cases as ct
import spectral_route_cases as routes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsp.jl_amd", "csrc", "ctbig_sizes.h")
LISTS = ("MDSP_CTBIG_LEAN_SIZES", "MDSP_CTBIG_SIZES", "MDSP_CTBIG_PREF_SIZES", "MDSP_CTBIG_SMALL_SIZES")


def _list_body(text, name):
    """the match of `#define <name>(X)` whose group 1 is the macro's body, continuation lines included"""
    m = re.search(r"#define\s+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
    assert m, name
    return m


def header_lists(path=HEADER):
    """{list name: set of sizes}: the X(N, ...) entries of each `#define MDSP_CTBIG_*SIZES(X)`"""
    text = open(path).read()
    out = {}
    for name in LISTS:
        m = _list_body(text, name)
        sizes = [int(n) for n in re.findall(r"X\(\s*(\d+)\s*,", m.group(1))]
        assert sizes and len(sizes) == len(set(sizes)), name
        out[name] = set(sizes)
    return out


def _sizes(cases):
    return {c.nfft for c in cases}


def _rows(cases):
    return {c.nfft // c.r0 for c in cases}


def check_header_against_cases(lists):
    union = set().union(*lists.values())
    assert sum(len(v) for v in lists.values()) == len(union)            # no size in two lists
    for dtype in (ct.F32, ct.C32):
        assert _sizes(ct.direct(ct.WELCH, dtype)) == union
        assert _sizes(ct.direct(ct.STFT, dtype)) == union - lists["MDSP_CTBIG_PREF_SIZES"]
        assert _rows(ct.rows(dtype, 6)) == lists["MDSP_CTBIG_SIZES"] | lists["MDSP_CTBIG_LEAN_SIZES"]
    for dtype in (ct.F64, ct.C64):
        assert _sizes(ct.direct(ct.WELCH, dtype)) <= union
        assert _sizes(ct.direct(ct.STFT, dtype)) <= union
        assert _rows(ct.rows(dtype, 7)) <= union
        assert _rows(ct.two_kernel_rows(dtype)) <= union


def test_header_lists_against_cases():
    lists = header_lists()
    assert [len(lists[name]) for name in LISTS] == [71, 6, 7, 93]
    check_header_against_cases(lists)


def test_counts():
    for dtype in ct.DTYPES:
        welch = ct.welch_cases(dtype)
        assert len(welch) == ct.WELCH_COUNTS[dtype], dtype
        assert max(c.nfft for c in welch) == ct.WELCH_LARGEST[dtype], dtype
        assert len(ct.direct(ct.STFT, dtype)) == ct.COLS_COUNTS[dtype], dtype
        for family in ct.FAMILIES:
            cases = ct.family_cases(family, dtype)
            assert len(cases) == len(set(cases)), (family, dtype)
            assert all(c.dtype == dtype and c.kind == (ct.STFT if family == "cols_direct" else ct.WELCH) for c in cases)
    everything = ct.all_cases()
    assert len(everything) == ct.TOTAL_CASES == sum(ct.WELCH_COUNTS.values()) + sum(ct.COLS_COUNTS.values())
    assert 25_000_000 < sum(c.nfft for c in everything) < 26_000_000
    # the direct families end at one workgroup's 16384 points, the rows at 2^19
    assert max(c.nfft for c in everything if c.route in (4, 5)) == 16384
    assert max(c.nfft for c in everything) < 1 << 19


def test_counts_of_the_route_table():
    """the figures the sweep's case lists are drawn from: sizes per route, distinct rows and distinct r0"""
    want = {  # (dtype, route): (sizes, distinct rows, r0s)
        (ct.F32, 6): (212, 77, (2, 3, 4, 5)), (ct.F32, 7): (0, 0, ()), (ct.F32, 8): (0, 0, ()),
        (ct.F64, 6): (0, 0, ()), (ct.F64, 7): (131, 59, (2, 3, 4)), (ct.F64, 8): (7, 4, (2, 3, 4)),
    }
    r9 = (6, 7, 8, 9, 10, 12, 14, 15, 16, 18, 20, 21, 24, 25, 27, 28, 30, 32)
    for cplx in (0, 2):
        for (dtype, route), (nsizes, nrows, r0s) in want.items():
            cs = ct.on_route(ct.WELCH, dtype + cplx, route)
            assert (len(cs), len(_rows(cs)), tuple(sorted({c.r0 for c in cs}))) == (nsizes, nrows, r0s), (dtype + cplx, route)
        assert len(ct.on_route(ct.WELCH, ct.F32 + cplx, 9)) == 395 and len(ct.on_route(ct.WELCH, ct.F64 + cplx, 9)) == 373
        assert tuple(c.r0 for c in sorted(ct.two_kernel_rows(ct.F32 + cplx), key=lambda c: c.r0)) == r9
        assert tuple(c.r0 for c in sorted(ct.two_kernel_rows(ct.F64 + cplx), key=lambda c: c.r0)) == (5,) + r9


def test_every_row_and_r0_of_the_route_table_is_covered():
    for dtype in ct.DTYPES:
        for route, cases in [(r, ct.rows(dtype, r)) for r in ct.FUSED_ROW_ROUTES] + [(ct.ROUTE_CTROWS, ct.two_kernel_rows(dtype))]:
            table = ct.on_route(ct.WELCH, dtype, route)
            assert set(cases) <= set(table)
            assert {c.r0 for c in cases} == {c.r0 for c in table}, (dtype, route)
            if route != ct.ROUTE_CTROWS:
                assert _rows(cases) == _rows(table), (dtype, route)
            for c in cases:        # each case is the smallest size with its row or with its r0
                assert (c.nfft == min(t.nfft for t in table if t.r0 == c.r0)
                        or c.nfft == min(t.nfft for t in table if t.nfft // t.r0 == c.nfft // c.r0)), c
        for kind in (ct.WELCH, ct.STFT):
            assert ct.direct(kind, dtype) == ct.on_route(kind, dtype, ct.ROUTE_CTBIG if kind == ct.WELCH else ct.ROUTE_CTBIG_COLS)


def test_case_lists_are_deterministic():
    assert ct.all_cases() == ct.all_cases()
    for dtype in ct.DTYPES:
        for family in ct.FAMILIES:
            assert ct.family_cases(family, dtype) == ct.family_cases(family, dtype)


def test_a_lost_header_entry_or_case_is_noticed(tmp_path, monkeypatch):
    """the check itself: one X(...) entry less in a copy of the header, or one case less from the generator, fails it"""
    text = open(HEADER).read()
    for name in LISTS:                     # the first entry of each list in turn
        body = _list_body(text, name)
        entry = re.search(r"X\(\s*\d+\s*,[^)]*\)", body.group(1))
        lo, hi = body.start(1) + entry.start(), body.start(1) + entry.end()
        copy = tmp_path / "ctbig_sizes.h"
        copy.write_text(text[:lo] + text[hi:])
        lists = header_lists(str(copy))
        assert len(lists[name]) == len(header_lists()[name]) - 1
        with pytest.raises(AssertionError):
            check_header_against_cases(lists)
    full = ct.on_route
    monkeypatch.setattr(ct, "on_route", lambda kind, dtype, route: [c for c in full(kind, dtype, route) if c.nfft != 12500 and c.nfft // max(c.r0, 1) != 12500])
    with pytest.raises(AssertionError):
        check_header_against_cases(header_lists())
    with pytest.raises(AssertionError):
        test_counts()


def test_window_is_asymmetric():
    for n in (1273, 1280, 16384, 497664):
        w = ct.window(n)
        assert w.dtype == np.float64 and w.shape == (n,)
        assert np.max(np.abs(w - w[::-1])) > 0.1 * np.max(w)
        half = n // 2      # ... and the halves differ in level
        assert abs(np.sum(w[:half] ** 2) - np.sum(w[n - half:] ** 2)) > 0.1 * np.sum(w ** 2)


def test_signal():
    for dtype in ct.DTYPES:
        dt = ct.NP_DTYPES[dtype]
        s = ct.signal(7, 4001, dt)
        assert s.dtype == dt and s.shape == (4001,)
        assert np.array_equal(s, ct.signal(7, 4001, dt)) and not np.array_equal(s, ct.signal(8, 4001, dt))
        if dt.kind == "c":
            assert abs(np.corrcoef(s.real, s.imag)[0, 1]) < 0.2          # an imaginary part of its own
        # the ramp: the last quarter is about 1.44 / 1.06 times the level of the first
        q = len(s) // 4
        assert 1.2 < np.sqrt(np.mean(np.abs(s[-q:]) ** 2) / np.mean(np.abs(s[:q]) ** 2)) < 1.5
    # Float32 types are rounded before the oracle sees them
    assert np.array_equal(ct.signal(3, 100, np.float32).astype(np.float64), ct.signal(3, 100, np.float64).astype(np.float32).astype(np.float64))
    # the tone is no bin centre of any case
    for nfft in sorted({c.nfft for c in ct.all_cases()}):
        b = ct.TONE / (2 * np.pi) * nfft
        assert abs(b - round(b)) > 1e-3, nfft


def test_configurations_give_the_frame_counts_asked_for():
    from oracle import periodograms as opg
    from dsp_jl_amd import _dev
    itemsize = {}
    for c in ct.all_cases():
        itemsize[c.nfft] = max(itemsize.get(c.nfft, 0), ct.NP_DTYPES[c.dtype].itemsize)
    for nfft in sorted(itemsize):
        a, b = ct.configs(nfft)
        assert (a.name, a.n, a.noverlap, a.frames, a.channels) == ("A", nfft, nfft // 2, 3, 1) and a.window.shape == (nfft,)
        assert (b.name, b.n, b.noverlap, b.frames, b.channels) == ("B", nfft - 7, (nfft - 7) // 3, 4, 2) and b.window is None
        for cfg in (a, b):
            assert 0 <= cfg.noverlap < cfg.n <= nfft
            assert cfg.length == (cfg.frames - 1) * (cfg.n - cfg.noverlap) + cfg.n + 5
            assert opg.frame_count(cfg.length, cfg.n, cfg.noverlap) == cfg.frames
            assert opg.frame_count(cfg.length - 6, cfg.n, cfg.noverlap) == cfg.frames - 1      # the five extra samples are a ragged tail, no frame
            # below the size from which host arrays take the library's host pipeline: the GPU test's calls run their plan on the device path
            assert cfg.length * cfg.channels * itemsize[nfft] < _dev.HOST_PIPELINE_MIN_BYTES
    case = ct.Case(ct.WELCH, ct.C32, 1280, 4, 0)
    a, b = ct.configs(1280)
    assert ct.case_signal(case, a).shape == (a.length,) and ct.case_signal(case, b).shape == (b.length, 2)
    sb = ct.case_signal(case, b)
    assert not np.array_equal(sb[:, 0], sb[:, 1]) and np.array_equal(sb, ct.case_signal(case, b))


def test_route_pin():
    """mdsp_spectral_route_for gives each case's (route, r0) with engine FUSED -- host arithmetic.  Skipped when the library is not built."""
    from dsp_jl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmi355dsp.so is not built")
    lib = _lib.lib()
    eng, route, r0 = C.c_int(), C.c_int(), C.c_int()
    bad = []
    for c in ct.all_cases():
        _lib.check(lib.mdsp_spectral_route_for(c.kind, c.dtype, c.nfft, ct.FUSED, C.byref(eng), C.byref(route), C.byref(r0)))
        if (eng.value, route.value, r0.value) != (ct.FUSED, c.route, c.r0):
            bad.append((c, eng.value, route.value, r0.value))
    assert not bad, f"{len(bad)} cases on another route (case, engine, route, r0), first: {bad[:10]}"
    assert (routes.ROUTE_CHARS[ct.ROUTE_CTROWS], routes.R0_ROUTES) == ("9", "6789")
