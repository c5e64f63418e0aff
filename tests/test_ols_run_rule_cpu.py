"""The run schedule of the fused overlap-save kernel (dsp.jl_amd/csrc/ols_plan.h ols_run_rule / ols_run_len, DESIGN.md 4.2 *Run schedule*) as pure host
arithmetic: mdsp_ols_run_for reports the run length and the iteration count launch_fused_geo gives a launch of `units` units on `slots` slots.  The
streaming launch of a tiled plan of at least FROM_UNITS units walks runs of RUN_UNITS units (never more than one run per slot holds); every other launch
walks one run per slot, WHOLE = ceil(units / slots), as before the rule.  The walk of ols_fused_kernel is replayed here: slot s starts at unit s run_len, walks run_len
consecutive units, then jumps slots x run_len ahead, niter iterations in all.  No device."""
import ctypes as C

import numpy as np
import pytest

from dsp_jl_amd import _lib

RUN_UNITS = 2               # the measured best length of the streaming tiled launch
FROM_UNITS = 1 << 16        # ... and the unit count from which it lost no round against one run per slot
HEADLINE = (299594, 1024)   # units and slots of 2^30 Float32 samples on 256 CUs x 4 workgroups: ceil(ceil(2^30 / 1792) / 2)


def _cdiv(a, b):
    return -(-a // b)


def run_for(units, slots, streaming):
    rl, ni = C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_ols_run_for(units, slots, 1 if streaming else 0, C.byref(rl), C.byref(ni)))
    return rl.value, ni.value


class _knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        _lib.set_tunable(self.name, self.value)

    def __exit__(self, *exc):
        _lib.set_tunable(self.name, None)


def _walk(units, slots, run_len, niter):
    """(times every unit is visited, dead iterations of every slot) under the kernel's walk (ols.hip OlsWalk / ols_walk_next)."""
    it = np.arange(niter)
    off = (it // run_len) * slots * run_len + it % run_len            # unit of slot 0 at iteration `it`
    u = off[None, :] + (np.arange(slots) * run_len)[:, None]
    live = u < units
    return np.bincount(u[live], minlength=units), niter - live.sum(axis=1)


def _check_schedule(units, slots, run_len, niter):
    whole = max(1, _cdiv(units, slots))
    assert 1 <= run_len <= whole
    assert niter % run_len == 0                                       # whole runs: every slot the same trip count
    assert niter == _cdiv(whole, run_len) * run_len                   # the smallest multiple of run_len that holds whole's iterations ...
    assert niter - whole < run_len                                    # ... so fewer than one run more than whole's
    visits, dead = _walk(units, slots, run_len, niter)
    assert visits.shape == (units,) and (visits == 1).all(), np.flatnonzero(visits != 1)[:8]
    assert dead.max() <= run_len, (dead.max(), run_len)               # a slot idles through at most one run


def _unit_counts(slots, run_len, base=0):
    """Prime counts, one below / at / one above slots x run_len (and twice that), fewer units than slots; base: the multiple of slots x run_len to start from."""
    full = slots * run_len
    grid = {base + u for u in (1, 2, slots - 1, slots, slots + 1, full - 1, full, full + 1, 2 * full - 1, 2 * full + 1, 7 * slots, 7 * slots + 1)}
    primes = {997, 7919, 104729 if slots >= 256 else 10007} if base == 0 else {65537, 104729}
    return sorted((grid | primes) - {0, -1})


@pytest.mark.parametrize("slots", [1, 3, 64, 256, 1024])
def test_other_launches_walk_one_run_per_slot(slots):
    for units in _unit_counts(slots, 3):
        run_len, niter = run_for(units, slots, False)
        assert run_len == niter == max(1, _cdiv(units, slots)), (units, slots)
        _check_schedule(units, slots, run_len, niter)


@pytest.mark.parametrize("slots", [64, 256, 1024, 1 << 16, 1 << 17])
def test_streaming_tiled_launches_walk_short_runs(slots):
    base = _cdiv(FROM_UNITS, slots * RUN_UNITS) * slots * RUN_UNITS
    for units in _unit_counts(slots, RUN_UNITS, base):
        assert units >= FROM_UNITS
        run_len, niter = run_for(units, slots, True)
        assert run_len == min(RUN_UNITS, max(1, _cdiv(units, slots))), (units, slots)
        _check_schedule(units, slots, run_len, niter)


@pytest.mark.parametrize("slots", [1, 3, 256, 1024])
def test_small_streaming_launches_walk_one_run_per_slot(slots):
    for units in [u for u in _unit_counts(slots, RUN_UNITS) if u < FROM_UNITS] + [37450, FROM_UNITS - 1]:      # 37450: 2^27 samples
        run_len, niter = run_for(units, slots, True)
        assert run_len == niter == max(1, _cdiv(units, slots)), (units, slots)
    assert run_for(FROM_UNITS, 1024, True) == (RUN_UNITS, 64) and run_for(74899, 1024, True) == (RUN_UNITS, 74)    # 74899: 2^28 samples


def test_headline_shape():
    units, slots = HEADLINE
    assert run_for(units, slots, False) == (293, 293)
    run_len, niter = run_for(units, slots, True)
    assert run_len == RUN_UNITS and niter == _cdiv(293, RUN_UNITS) * RUN_UNITS
    _check_schedule(units, slots, run_len, niter)


def test_no_units():
    for streaming in (False, True):
        assert run_for(0, 64, streaming) == (1, 0)


@pytest.mark.parametrize("forced", [1, 2, 3, 7, 1 << 20])
@pytest.mark.parametrize("streaming", [False, True], ids=["plain", "streaming"])
def test_forced_run_length(forced, streaming):
    with _knob("MDSP_OLS_RUN_LEN", forced):
        for slots in (3, 256):
            for units in _unit_counts(slots, min(forced, 8)):
                run_len, niter = run_for(units, slots, streaming)
                assert run_len == min(forced, max(1, _cdiv(units, slots))), (units, slots)      # never longer than one run per slot
                _check_schedule(units, slots, run_len, niter)
    assert run_for(*HEADLINE, False) == (293, 293)                                               # the knob is back


def test_runs_per_slot_wins():
    units, slots = 7 * 256 - 4, 256
    with _knob("MDSP_RUNS_PER_SLOT", 2):
        for streaming in (False, True):
            assert run_for(units, slots, streaming) == (4, 8)
            with _knob("MDSP_OLS_RUN_LEN", 1):
                assert run_for(units, slots, streaming) == (4, 8)
    with _knob("MDSP_RUNS_PER_SLOT", 1):                                                         # the default value: the rule
        assert run_for(units, slots, False) == (7, 7)
        assert run_for(units, slots, True) == (7, 7)                                             # below FROM_UNITS
        assert run_for(HEADLINE[0], HEADLINE[1], True)[0] == RUN_UNITS


def test_argument_errors():
    rl, ni = C.c_int64(0), C.c_int64(0)
    assert _lib.lib().mdsp_ols_run_for(-1, 4, 0, C.byref(rl), C.byref(ni)) == _lib.ERR_ARGUMENT
    assert _lib.lib().mdsp_ols_run_for(10, 0, 0, C.byref(rl), C.byref(ni)) == _lib.ERR_ARGUMENT
    assert _lib.lib().mdsp_ols_run_for(10, 4, 1, None, None) == _lib.OK
