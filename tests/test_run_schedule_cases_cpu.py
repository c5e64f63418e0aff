"""The case tables of tests/run_schedule_cases.py against the properties tests/test_gpu_run_schedules.py relies on, without a GPU: every case gives
each slot a run of at least three units, a partial last run and an idle slot, MDSP_RUNS_PER_SLOT gives some slot a second run, every SHIFT case meets
the host's dispatch condition for the register-carry kernels and every control misses it.  Someone who changes a kernel geometry changes
run_schedule_cases.geometry with it; if a case then no longer reaches the code it is there for, this fails instead of the GPU tests passing quietly."""
import numpy as np
import pytest

import run_schedule_cases as rs

CUS = rs.CU_COUNTS


def _check_schedule(nunits, nslots, runs2):
    run_len, niter = rs.schedule(nunits, nslots, 1)
    assert run_len >= 3
    assert nunits % run_len != 0                              # the last run is partial
    nruns = -(-nunits // run_len)
    assert nruns < nslots                                     # at least one slot has nothing to do
    assert niter == run_len                                   # one run per slot
    assert rs.runs_of_slot(nunits, nslots, 1, nslots - 1) == []
    last = rs.runs_of_slot(nunits, nslots, 1, nruns - 1)
    assert len(last) == 1 and 0 < last[0][1] - last[0][0] < run_len
    # more runs per slot: shorter runs, and some slot walks two of them (the schedule's trip count covers the second)
    rl2, niter2 = rs.schedule(nunits, nslots, runs2)
    assert 2 <= rl2 < run_len
    assert niter2 >= 2 * rl2
    two = [s for s in range(nslots) if len(rs.runs_of_slot(nunits, nslots, runs2, s)) >= 2]
    assert two
    first, second = rs.runs_of_slot(nunits, nslots, runs2, two[0])[:2]
    assert second[0] == first[0] + nslots * rl2 and second[0] != first[1]      # the second run does not continue the first
    # every unit is walked exactly once
    for runs in (1, runs2):
        seen = sorted(u for s in range(nslots) for a, b in rs.runs_of_slot(nunits, nslots, runs, s) for u in range(a, b))
        assert seen == list(range(nunits))


def test_schedule_is_the_hosts_formula():
    # set_schedule: run_len = max(1, cdiv(nunits, nslots * runs)), niter = cdiv(cdiv(nunits, run_len), nslots) * run_len
    assert rs.schedule(100, 512, 1) == (1, 1)                 # fewer units than slots: what the rest of the suite runs
    assert rs.schedule(512, 512, 1) == (1, 1)
    assert rs.schedule(513, 512, 1) == (2, 2)
    assert rs.schedule(1532, 512, 1) == (3, 3)
    assert rs.schedule(1532, 512, 2) == (2, 4)
    assert rs.schedule(1, 1, 1) == (1, 1)
    assert rs.schedule(7, 1, 3) == (3, 9)
    assert rs.units_for(512) == 1532


def test_geometry_mirrors_the_launchers():
    g = rs.geometry
    # Geo<R, N> (spectral_op.h): 8 elements per thread, 16 at Float32 nfft 1024, whole wavefronts; several one-wave transforms share a workgroup
    assert [g("stft", rs.C32, n) for n in (256, 512, 1024, 2048, 4096, 8192)] == [(4, 64, 4), (8, 64, 4), (16, 64, 4), (8, 256, 1), (8, 512, 1), (8, 1024, 1)]
    assert [g("stft", rs.F64, n) for n in (256, 512, 1024, 2048, 4096)] == [(4, 64, 4), (8, 64, 4), (8, 128, 1), (8, 256, 1), (8, 512, 1)]
    assert g("welch", rs.C32, 4096) == (8, 512, 1) and g("welch", rs.F32, 4096) == (16, 256, 1) and g("welch", rs.F64, 4096) == (8, 512, 1)
    assert [g("welch_half", rs.F32, n) for n in (1024, 2048, 4096, 8192)] == [(16, 64, 4), (16, 128, 1), (16, 256, 1), (16, 512, 1)]
    assert g("welch_half", rs.F64, 2048) == (8, 256, 1)
    # launch_fused_n (ols.hip): 16 elements per thread for Float32 from nfft 1024 on; real Float32 nfft 2048 one transform per workgroup
    assert [g("ols", rs.F32, n) for n in (256, 512, 1024, 2048, 4096, 8192)] == [(4, 64, 4), (8, 64, 4), (16, 64, 4), (16, 128, 1), (16, 256, 1), (16, 512, 1)]
    assert g("ols", rs.C32, 2048) == (16, 128, 1) and g("ols", rs.F64, 1024) == (8, 128, 1) and g("ols", rs.C64, 512) == (8, 64, 4)


@pytest.mark.parametrize("cu", CUS)
def test_spectral_cases_give_every_slot_a_run(cu):
    for op, cases in (("stft", rs.STFT_SHIFT_CASES), ("welch", rs.WELCH_SHIFT_CASES)):
        for nfft, sh in cases:
            _, _, G = rs.geometry(op, rs.C32, nfft)
            ns = rs.slots(cu, rs.NCH, G, op)
            _check_schedule(rs.units_for(ns), ns, 2)          # complex signals: a unit is a frame
        for _, dt, nfft, _, _ in rs.control_cases(op):
            _, _, G = rs.geometry(op, dt, nfft)
            ns = rs.slots(cu, rs.NCH, G, op)
            _check_schedule(rs.units_for(ns), ns, 2)
    for dt, nfft in rs.REAL_CASES:
        kinds = {"stft"} | {kind for _, kind, _, _ in rs.real_welch_forms(nfft)}
        for kind in kinds:
            _, _, G = rs.geometry(kind, dt, nfft)
            ns = rs.slots(cu, rs.NCH, G, kind)
            K = rs.real_frames(ns)
            assert K % 2 == 1 and (K + 1) // 2 == rs.units_for(ns)      # frame pairs; the last unit carries one frame
            _check_schedule((K + 1) // 2, ns, 2)


@pytest.mark.parametrize("cu", CUS)
def test_overlap_save_cases_give_every_slot_a_run(cu):
    for dt, nfft in rs.OLS_CASES:
        nb, L, nblocks, nx, upc, ns = rs.ols_shape(dt, nfft, cu)
        assert ns == cu * rs.geometry("ols", dt, nfft)[2]
        assert nb == nfft // 8 + 1 and L == nfft - nb + 1
        assert -(-nx // L) == nblocks and nx % L != 0                   # the column's last block is partial
        if np.dtype(dt).kind == "c":
            assert upc == nblocks
        else:
            assert nblocks % 2 == 1 and upc == (nblocks + 1) // 2       # the column's last unit has one block
        assert 0 <= upc * rs.OLS_NCOLS - rs.units_for(ns) <= 4 * rs.OLS_NCOLS   # as close to units_for as three equal columns with a partial run get
        _check_schedule(upc * rs.OLS_NCOLS, ns, rs.OLS_RUNS)
        # runs cross column boundaries (the kernel recovers column and position from the unit number)
        run_len, _ = rs.schedule(upc * rs.OLS_NCOLS, ns, 1)
        assert upc % run_len != 0


def test_shift_cases_meet_the_dispatch_condition():
    assert len(rs.STFT_SHIFT_CASES) == 16 and len(rs.WELCH_SHIFT_CASES) == 15
    assert (1024, 8) in rs.STFT_SHIFT_CASES and (1024, 8) not in rs.WELCH_SHIFT_CASES
    for op, cases in (("stft", rs.STFT_SHIFT_CASES), ("welch", rs.WELCH_SHIFT_CASES)):
        assert len(set(cases)) == len(cases)
        for nfft, sh in cases:
            dt, nfft_, n, hop = rs.shift_case(op, nfft, sh)
            E, T, _ = rs.geometry(op, dt, nfft)
            assert dt == rs.C32 and nfft_ == nfft
            assert n == nfft and hop % T == 0 and hop // T == sh < E and E > 4
            assert 0 < hop < n
            assert rs.carry_shift(op, dt, nfft, n, hop) == sh


def test_controls_miss_the_dispatch_condition():
    for op in ("stft", "welch"):
        ids = [c[0] for c in rs.control_cases(op)]
        assert len(set(ids)) == len(ids)
        for cid, dt, nfft, n, hop in rs.control_cases(op):
            assert 0 < hop <= n <= nfft, cid
            assert rs.carry_shift(op, dt, nfft, n, hop) == 0, cid
            E, T, _ = rs.geometry(op, dt, nfft)
            assert not (np.dtype(dt) == rs.C32 and n == nfft and hop % T == 0 and hop // T < E and E > 4
                        and hop // T in ((1, 2, 4, 8) if (op == "stft" and E > 8) else (1, 2, 4))), cid
    # every way of missing it is there
    kinds = {cid.split("-", 1)[1] for cid, *_ in rs.control_cases("stft")}
    assert kinds >= {"no-overlap", "hop-1.5T", "n-short", "E4", "ComplexF64"}
    # the same shapes with ComplexF32 and the carry's hop would take it: the controls sit on the edge, not far from it
    assert rs.carry_shift("stft", rs.C32, 1024, 1024, 256) == 4 and rs.carry_shift("stft", rs.C32, 1024, 1024, 512) == 8
    assert rs.carry_shift("welch", rs.C32, 1024, 1024, 256) == 4 and rs.carry_shift("welch", rs.C32, 1024, 1024, 512) == 0


def test_real_forms_take_the_kernels_they_name():
    for dt, nfft in rs.REAL_CASES:
        forms = {fid: (kind, n, hop) for fid, kind, n, hop in rs.real_welch_forms(nfft)}
        kind, n, hop = forms["half"]
        assert kind == "welch_half" and n == nfft and 2 * hop == nfft          # welch_launch_n: `a.n == N && 2 * a.hop == N`
        for fid in ("quarter", "ztail"):
            kind, n, hop = forms[fid]
            assert kind == "welch" and not (n == nfft and 2 * hop == nfft) and 0 < hop < n <= nfft
        assert forms["ztail"][1] == nfft - 3 and forms["ztail"][2] == (nfft - 3) // 3
        for fid, n, hop, onesided in rs.real_stft_forms(nfft):
            assert 0 < hop < n <= nfft                                         # stft_launch_n: pairs whenever n <= N
        assert {o for *_, o in rs.real_stft_forms(nfft)} == {True, False}
