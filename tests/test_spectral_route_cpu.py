"""mdsp_spectral_route_for -- the kernel family a Welch / STFT / multitaper plan records at creation -- against the table of
tests/spectral_route_cases.py: every 7-smooth nfft to 2^20 and a few beyond, the four dtypes, both kinds and the three engines at the default tunables,
and the sizes where a route changes under each MDSP_GX / MDSP_BIGFFT setting.  Pure host arithmetic: no device needed."""
import ctypes as C

import pytest

from dsp_jl_amd import _lib

import spectral_route_cases as cases


def _check(table, sizes, engines):
    lib = _lib.lib()
    bad = []
    assert {key[2] for key in table} == set(engines)
    for (kind, dtype, engine), want in table.items():
        got = cases.encode(lib, kind, dtype, engine, sizes)
        for name, w, g in (("route", want[0], got[0]), ("r0", want[1], got[1])):
            assert len(w) == len(sizes)
            bad += [(kind, dtype, engine, n, name, a, b) for n, a, b in zip(sizes, w, g) if a != b]
    assert not bad, f"{len(bad)} differences (kind, dtype, engine, nfft, field, want, got), first: {bad[:10]}"


def test_routes_at_default_tunables():
    assert len(cases.DEFAULT) == len(cases.KINDS) * len(cases.DTYPES) * len(cases.ENGINES)
    _check(cases.expected_default(), cases.SIZES, cases.ENGINES)


@pytest.mark.parametrize("name,value", cases.KNOB_SETTINGS)
def test_routes_under_knob(name, value):
    table = cases.expected_knob((name, value))
    assert len(table) == len(cases.KINDS) * len(cases.DTYPES) * len(cases.KNOB_ENGINES)
    _lib.set_tunable(name, value)
    try:
        _check(table, cases.KNOB_SIZES, cases.KNOB_ENGINES)
    finally:
        _lib.set_tunable(name, None)


def test_route_query_arguments():
    lib = _lib.lib()
    eng, route, r0 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(lib.mdsp_spectral_route_for(0, _lib.F32, 4096, 1, None, None, None))   # any output may be NULL
    _lib.check(lib.mdsp_spectral_route_for(0, _lib.F32, 4096, 2, C.byref(eng), C.byref(route), C.byref(r0)))
    assert (eng.value, route.value, r0.value) == (2, 0, 0)
    with pytest.raises(_lib.ArgumentError):
        _lib.check(lib.mdsp_spectral_route_for(2, _lib.F32, 4096, 0, None, None, None))
    with pytest.raises(_lib.ArgumentError):
        _lib.check(lib.mdsp_spectral_route_for(0, 7, 4096, 0, None, None, None))
    with pytest.raises(_lib.ArgumentError, match="invalid engine 9"):
        _lib.check(lib.mdsp_spectral_route_for(1, _lib.F32, 4096, 9, None, None, None))
    # the error plan creation raises for a size no fused kernel takes
    with pytest.raises(_lib.UnsupportedError, match="fused engine supports nfft"):
        _lib.check(lib.mdsp_spectral_route_for(1, _lib.F64, 4099, 1, None, None, None))
