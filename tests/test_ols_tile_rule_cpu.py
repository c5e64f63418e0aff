"""The tile rule of the overlap-save plans (dsp.jl_amd/csrc/ols.hip ols_tile_rule) as pure host arithmetic: mdsp_ols_tile_for reports the
windows the whole-column call runs -- (tile, lead) == (L, nb - 1) for every plan except real Float32 plans of the fused engine at nfft 2048 whose filter
leaves at most P_MAX of the 256 lead samples unused: those run windows of 1792 outputs that start 256 samples early.  The public block grid
(mdsp_ols_geometry_for) does not move.  No device."""
import ctypes as C

import pytest

from dsp_jl_amd import _lib

P_MAX = 8           # the largest power of two p with p / 1793 <= g / 2, g the measured gain of the filter stage at p = 1
NFFT, TILE, LEAD = 2048, 1792, 256
NX = 1 << 20


def tile_for(nb, nfft, dtype=_lib.F32, mode=_lib.OLS_FILT, engine=_lib.ENGINE_AUTO, nx=NX):
    t, l = C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_ols_tile_for(nb, nfft, nx, dtype, mode, engine, C.byref(t), C.byref(l)))
    return t.value, l.value


def geometry_for(nb, nfft, dtype=_lib.F32, mode=_lib.OLS_FILT, engine=_lib.ENGINE_AUTO, nx=NX):
    en, el, ep, eg, er = C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().mdsp_ols_geometry_for(nb, nfft, nx, dtype, mode, engine, C.byref(en), C.byref(el), C.byref(ep), C.byref(eg), C.byref(er)))
    return en.value, el.value, ep.value, eg.value, er.value


# (nb, nfft, dtype, engine): plans the rule must leave alone
UNTILED = [(256, NFFT, _lib.F64, _lib.ENGINE_AUTO), (256, NFFT, _lib.C32, _lib.ENGINE_AUTO), (256, NFFT, _lib.F32, _lib.ENGINE_ROCFFT),
           (256, 1024, _lib.F32, _lib.ENGINE_AUTO), (256, 4096, _lib.F32, _lib.ENGINE_AUTO), (129, NFFT, _lib.F32, _lib.ENGINE_AUTO),
           (300, NFFT, _lib.F32, _lib.ENGINE_AUTO)]
PARTITIONED = (6000, 16384, _lib.F32, _lib.ENGINE_FUSED)      # 2 partitions of 4096 taps: windows of exec_nfft / 2


def _all_cases():
    cases = [(256, NFFT, _lib.F32, mode, eng) for mode in (_lib.OLS_FILT, _lib.OLS_CONV) for eng in (_lib.ENGINE_AUTO, _lib.ENGINE_FUSED)]
    cases += [(nb, nfft, dt, _lib.OLS_FILT, eng) for nb, nfft, dt, eng in UNTILED + [PARTITIONED]]
    cases += [(nb, NFFT, _lib.F32, _lib.OLS_FILT, _lib.ENGINE_AUTO) for nb in range(225, 258)]
    return cases


def test_headline_shape_is_tiled():
    for mode in (_lib.OLS_FILT, _lib.OLS_CONV):
        for eng in (_lib.ENGINE_AUTO, _lib.ENGINE_FUSED):
            assert tile_for(256, NFFT, mode=mode, engine=eng) == (TILE, LEAD), (mode, eng)


@pytest.mark.parametrize("nb,nfft,dtype,engine", UNTILED)
def test_other_plans_keep_their_blocks(nb, nfft, dtype, engine):
    assert tile_for(nb, nfft, dtype, engine=engine) == (nfft - nb + 1, nb - 1)


def test_partitioned_plan_keeps_its_blocks():
    nb, nfft, dt, eng = PARTITIONED
    en, el, parts, _, _ = geometry_for(nb, nfft, dt, engine=eng)
    assert parts > 1 and el == en // 2
    assert tile_for(nb, nfft, dt, engine=eng) == (el, nb - 1)


def test_tiled_exactly_up_to_p_max():
    assert P_MAX >= 1 and P_MAX & (P_MAX - 1) == 0
    for nb in range(225, 258):
        p = LEAD - (nb - 1)
        want = (TILE, LEAD) if p <= P_MAX else (NFFT - nb + 1, nb - 1)
        assert tile_for(nb, NFFT) == want, (nb, p)


def test_public_geometry_does_not_move_and_the_knob_switches_the_rule_off():
    cases = _all_cases()
    before = [geometry_for(nb, nfft, dt, mode, eng) for nb, nfft, dt, mode, eng in cases]
    assert geometry_for(256, NFFT) == (2048, 1793, 1, _lib.ENGINE_FUSED, 0)
    try:
        _lib.set_tunable("MDSP_OLS_TILE", 0)
        for (nb, nfft, dt, mode, eng), geo in zip(cases, before):
            assert tile_for(nb, nfft, dt, mode, eng) == (geo[1], nb - 1), (nb, nfft, dt, mode, eng)
            assert geometry_for(nb, nfft, dt, mode, eng) == geo
    finally:
        _lib.set_tunable("MDSP_OLS_TILE", None)
    assert tile_for(256, NFFT) == (TILE, LEAD)
    assert [geometry_for(nb, nfft, dt, mode, eng) for nb, nfft, dt, mode, eng in cases] == before
