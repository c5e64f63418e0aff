"""Case table of the chunk-seam tests (tests/test_gpu_chunk_seams.py): for every engine loop that cuts its work into chunks to keep its intermediates
within a memory budget, the smallest shapes that cross the budget -- and what each case exists for.  No device: tests/test_chunk_cases_cpu.py holds the
table to the library's own host arithmetic (mdsp_chunk_units_for under the case's knobs, mdsp_spectral_route_for, mdsp_ols_geometry_for), so that a changed
budget or route fails there instead of quietly taking the GPU tests back to one chunk.

The loops (dsp.jl_amd/csrc) and their budgets:

    loop              where                                   budget                                 a unit
    rocfft_welch      welch.hip welch_accumulate_rocfft       MDSP_ROCFFT_CHUNK_MIB (192)            a frame of a channel
    rocfft_stft       stft.hip stft_exec_rocfft               the same                               a frame of a channel
    rocfft_ols        ols.hip exec_rocfft                     64 MiB, fixed                          a block of a column
    hilbert           hilbert.hip hilbert_run                 256 MiB, fixed                         a column
    big_welch         bigfft.hip run, mode 0                  MDSP_BIG_CHUNK_MIB (1024)              a transform: two real frames, one complex frame
    big_cols          bigfft.hip run, mode 1                  the same                               the same
    big_welch_rows    bigfft.hip run_welch_rows               the same                               the same
    big_ols           bigfft.hip run_ols                      the same, two buffers                  a transform: two real blocks, one complex block
    big_ols_rows      bigfft.hip run_ols_rows                 the same                               the same

A case names the knobs set while its plan is made (`create`: the route) and around its calls (`launch`: the budget), its shape, and in `expect` the chunk
schedule its call must have: the number of chunks, the size of the last one, and the properties that are the point of the case --

    spans      a chunk starts in one channel (column) and ends in the next
    one_frame  the last unit holds one frame (block) of a real signal
    slices     (chunks, last) of every accumulate call of a streaming case
    ref_chunks the chunk count of the same call under the launch knobs of `ref` (the default budget: one chunk), against which the GPU test compares

Where the knobs allow it a case has two full chunks and a shorter last one; the cases that are fixed at one unit per chunk (C = 1) have three chunks of one."""
from collections import namedtuple

import numpy as np

F32, F64, C32, C64 = 0, 1, 2, 3
NP_DTYPE = {F32: np.float32, F64: np.float64, C32: np.complex64, C64: np.complex128}
AUTO, FUSED, ROCFFT = 0, 1, 2
OLS_FILT, OLS_CONV = 0, 1
ROUTE_ROCFFT, ROUTE_BIG = 0, 10
# MDSP_CHUNK_* of include/mi355dsp.h
CHUNK_ROCFFT_WELCH, CHUNK_ROCFFT_STFT, CHUNK_ROCFFT_OLS, CHUNK_HILBERT, CHUNK_BIG_SPECTRAL, CHUNK_BIG_OLS, CHUNK_BIG_OLS_ROWS = range(7)

LOOPS = ("rocfft_welch", "rocfft_stft", "rocfft_ols", "hilbert", "big_welch", "big_cols", "big_welch_rows", "big_ols", "big_ols_rows")
LOOP_KIND = {"rocfft_welch": CHUNK_ROCFFT_WELCH, "rocfft_stft": CHUNK_ROCFFT_STFT, "rocfft_ols": CHUNK_ROCFFT_OLS, "hilbert": CHUNK_HILBERT,
             "big_welch": CHUNK_BIG_SPECTRAL, "big_cols": CHUNK_BIG_SPECTRAL, "big_welch_rows": CHUNK_BIG_SPECTRAL, "big_ols": CHUNK_BIG_OLS,
             "big_ols_rows": CHUNK_BIG_OLS_ROWS}

Case = namedtuple("Case", "id loop dtype op create launch shape expect")


def is_complex(dtype):
    return dtype in (C32, C64)


def is_double(dtype):
    return dtype in (F64, C64)


def dt_name(dtype):
    return np.dtype(NP_DTYPE[dtype]).name


# ---- spectral cases ----------------------------------------------------------------------------------------------------------------------------------
# op: "welch" (mdsp_welch_exec), "stream" (reset / accumulate per slice / finalize), "stft" (raw columns), "psd" (psd_only columns: spectrogram),
#     "mt" (mdsp_mt_psd_exec: one pass over all units per taper, the accumulate flag set from the second taper on)
# shape: nfft, n, noverlap, K frames per channel (one call), nch, onesided, ldo_pad (column stride = nout + ldo_pad), slices (frames per accumulate call),
#        ntapers / nw (mt)
def _spec(id, loop, dtype, op, nfft, n, noverlap, K, nch, expect, onesided=None, ldo_pad=0, create=None, launch=None, slices=None, ntapers=0, nw=0.0, window="hanning"):
    onesided = (not is_complex(dtype)) if onesided is None else onesided
    shape = dict(nfft=nfft, n=n, noverlap=noverlap, K=K, nch=nch, onesided=onesided, ldo_pad=ldo_pad, slices=slices, ntapers=ntapers, nw=nw, window=window)
    return Case(id, loop, dtype, op, create or {}, launch or {}, shape, expect)


def _e(chunks, last, spans=False, one_frame=False, ref_chunks=1):
    return dict(chunks=chunks, last=last, spans=spans, one_frame=one_frame, ref_chunks=ref_chunks)


ROC1 = {"MDSP_ROCFFT_CHUNK_MIB": 1}
# nfft 1000 = 2^3 5^3 under a budget of 1 MiB: 130 Float32 frames per chunk (8008 bytes each: 1000 samples and 501 bins), 65 Float64 or ComplexF32, 32 ComplexF64.
# 97 frames per channel: a prime no chunk size divides.  Float32: 3 channels, 291 units = 130 + 130 + 31, chunk 0 ends 33 frames into channel 1, chunk 1 covers the
# rest of channel 1 and 66 frames of channel 2.  The others: 2 channels, 194 units = 65 + 65 + 64 (ComplexF64: six chunks of 32 and one of 2).
# n = 960 < nfft: every frame has a zero tail; 50 % overlap.
_RN, _RNFFT, _RK = 960, 1000, 97


def _roc_expect(dtype):
    return {F32: _e(3, 31, spans=True, one_frame=False), F64: _e(3, 64, spans=True), C32: _e(3, 64, spans=True), C64: _e(7, 2, spans=True)}[dtype]


def _roc_nch(dtype):
    return 3 if dtype == F32 else 2


ROCFFT_SPECTRAL = []
for _dt in (F32, F64, C32, C64):
    _sides = (False,) if is_complex(_dt) else (True, False)
    for _one in _sides:
        _s = "" if is_complex(_dt) else ("-onesided" if _one else "-twosided")
        ROCFFT_SPECTRAL.append(_spec(f"rocfft-welch-{dt_name(_dt)}{_s}", "rocfft_welch", _dt, "welch", _RNFFT, _RN, _RN // 2, _RK, _roc_nch(_dt), _roc_expect(_dt),
                                     onesided=_one, launch=ROC1))
        # raw STFT, the direct layout (column stride nout == the transform's own nspec, channels back to back): full chunks are transformed straight into the
        # output, the shorter last chunk goes through stft_store_kernel behind them.  Two-sided real output is never direct (nout != nspec).
        ROCFFT_SPECTRAL.append(_spec(f"rocfft-stft-{dt_name(_dt)}{_s}-packed", "rocfft_stft", _dt, "stft", _RNFFT, _RN, _RN // 2, _RK, _roc_nch(_dt), _roc_expect(_dt),
                                     onesided=_one, launch=ROC1))
    # ldo > nout: no chunk is direct
    ROCFFT_SPECTRAL.append(_spec(f"rocfft-stft-{dt_name(_dt)}-strided", "rocfft_stft", _dt, "stft", _RNFFT, _RN, _RN // 2, _RK, _roc_nch(_dt), _roc_expect(_dt), ldo_pad=3,
                                 launch=ROC1))
    ROCFFT_SPECTRAL.append(_spec(f"rocfft-psd-{dt_name(_dt)}", "rocfft_stft", _dt, "psd", _RNFFT, _RN, _RN // 2, _RK, _roc_nch(_dt), _roc_expect(_dt), ldo_pad=3, launch=ROC1))
ROCFFT_SPECTRAL += [
    # multitaper on this engine: one chunked pass per taper into the same columns.  mt_pgram is the one-frame call (K = 1): its units are the channels.
    _spec("rocfft-mt-pgram-float32", "rocfft_stft", F32, "mt", _RNFFT, _RN, 0, 1, 291, _e(3, 31, spans=True), launch=ROC1, ntapers=3, nw=2.0, window=None),
    _spec("rocfft-mt-spectrogram-float32", "rocfft_stft", F32, "mt", _RNFFT, _RN, _RN // 2, _RK, 3, _e(3, 31, spans=True), launch=ROC1, ntapers=3, nw=2.0, window=None),
    _spec("rocfft-mt-spectrogram-complex128", "rocfft_stft", C64, "mt", _RNFFT, _RN, _RN // 2, _RK, 2, _e(7, 2, spans=True), launch=ROC1, ntapers=3, nw=2.0, window=None),
]

# Multi-pass engine, 16384 points (two passes of 128): 128 KiB per Float32 transform, so 8 per MiB (Float64: 4).  MDSP_GX = 0 while the plan is made: without it
# the single-workgroup schedules take this size in Float32.  The engine runs channel by channel, so no chunk spans channels; two channels check that the
# second one starts from the same state.
BIG_CREATE = {"MDSP_GX": 0}
BIG1 = {"MDSP_BIG_CHUNK_MIB": 1}
_BN = 16384
BIG_SPECTRAL = [
    # real, odd frame count: units = 2 C + 1, the last chunk is one unit holding one frame -- and takes the `groups == 1` branch, straight into the accumulator
    _spec("big-welch-float32-33", "big_welch", F32, "welch", _BN, _BN, _BN // 2, 33, 2, _e(3, 1, one_frame=True), create=BIG_CREATE, launch=BIG1),
    _spec("big-welch-float32-42-twosided", "big_welch", F32, "welch", _BN, _BN, _BN // 2, 42, 1, _e(3, 5), onesided=False, create=BIG_CREATE, launch=BIG1),
    _spec("big-welch-complex64-21", "big_welch", C32, "welch", _BN, _BN - 1000, _BN // 2, 21, 1, _e(3, 5), create=BIG_CREATE, launch=BIG1),
    _spec("big-welch-float64-17", "big_welch", F64, "welch", _BN, _BN, _BN // 2, 17, 1, _e(3, 1, one_frame=True), create=BIG_CREATE, launch=BIG1),
    _spec("big-welch-complex128-11", "big_welch", C64, "welch", _BN, _BN, _BN // 2, 11, 1, _e(3, 3), create=BIG_CREATE, launch=BIG1),
    # three passes (64 x 64 x 128, CASES of tests/test_gpu_bigfft.py) at one unit of 4 MiB per chunk; MDSP_BIG_WELCH_ROWS = 0 keeps the Welch sums off the rows form
    _spec("big-welch-float32-three-pass", "big_welch", F32, "welch", 524288, 262144, 131072, 5, 1, _e(3, 1, one_frame=True), create=BIG_CREATE,
          launch={"MDSP_BIG_CHUNK_MIB": 4, "MDSP_BIG_WELCH_ROWS": 0}),
    # the streaming form: 34 frames (17 units: 8 + 8 + 1), then 20 more (10 units: 8 + 2) on top of them -- each call is chunked, the second starts adding
    _spec("big-welch-float32-stream", "big_welch", F32, "stream", _BN, _BN, _BN // 2, 54, 1, dict(_e(3, 1), slices=((3, 1), (2, 2))), create=BIG_CREATE, launch=BIG1, slices=(34, 20)),
    # columns
    _spec("big-stft-float32-33", "big_cols", F32, "stft", _BN, _BN, _BN // 2, 33, 2, _e(3, 1, one_frame=True), create=BIG_CREATE, launch=BIG1),
    _spec("big-stft-float32-42-twosided", "big_cols", F32, "stft", _BN, _BN - 1000, _BN // 2, 42, 1, _e(3, 5), onesided=False, ldo_pad=3, create=BIG_CREATE, launch=BIG1),
    _spec("big-psd-float32-33", "big_cols", F32, "psd", _BN, _BN, _BN // 2, 33, 1, _e(3, 1, one_frame=True), ldo_pad=3, create=BIG_CREATE, launch=BIG1),
    _spec("big-stft-complex64-21", "big_cols", C32, "stft", _BN, _BN, _BN // 2, 21, 1, _e(3, 5), create=BIG_CREATE, launch=BIG1),
    _spec("big-stft-float64-17", "big_cols", F64, "stft", _BN, _BN, _BN // 2, 17, 1, _e(3, 1, one_frame=True), create=BIG_CREATE, launch=BIG1),
    _spec("big-psd-complex128-11", "big_cols", C64, "psd", _BN, _BN, _BN // 2, 11, 1, _e(3, 3), create=BIG_CREATE, launch=BIG1),
    _spec("big-stft-float32-three-pass", "big_cols", F32, "stft", 524288, 262144, 131072, 5, 1, _e(3, 1, one_frame=True), create=BIG_CREATE,
          launch={"MDSP_BIG_CHUNK_MIB": 4}),
    # multitaper spectrogram: PSD columns with the accumulate flag, through big_untangle_kernel (real) and the last pass itself (complex), at c0 > 0
    _spec("big-mt-spectrogram-float32", "big_cols", F32, "mt", _BN, _BN, _BN // 2, 33, 1, _e(3, 1, one_frame=True), create=BIG_CREATE, launch=BIG1, ntapers=3, nw=2.0,
          window=None),
    _spec("big-mt-spectrogram-complex64", "big_cols", C32, "mt", _BN, _BN, _BN // 2, 21, 1, _e(3, 5), create=BIG_CREATE, launch=BIG1, ntapers=3, nw=2.0, window=None),
    # Welch sums in the rows form (column pass + the single-workgroup Welch kernel over 64 rows): 64 x 8192 Float32 and 64 x 4096 Float64 are 4 MiB per
    # transform, two per chunk at 8 MiB; 9 real frames are 5 units = 2 + 2 + 1, and the row plan is accumulated into three times within the call
    _spec("big-welch-rows-float32", "big_welch_rows", F32, "welch", 64 * 8192, 64 * 8192, 32 * 8192, 9, 1, _e(3, 1, one_frame=True), create=BIG_CREATE,
          launch={"MDSP_BIG_CHUNK_MIB": 8}),
    _spec("big-welch-rows-float64", "big_welch_rows", F64, "welch", 64 * 4096, 64 * 4096, 32 * 4096, 9, 1, _e(3, 1, one_frame=True), create=BIG_CREATE,
          launch={"MDSP_BIG_CHUNK_MIB": 8}),
]
SPECTRAL = ROCFFT_SPECTRAL + BIG_SPECTRAL


def welch_rows_r0(dtype, nfft):
    """The row count of the multi-pass engine's rows form (bigfft.hip rows_r0: nfft = R0 x the longest single-workgroup transform, R0 in 32 .. 256), which
    the library does not report for Welch plans; 0: three passes."""
    S = 4096 if is_double(dtype) else 8192
    return nfft // S if nfft % S == 0 and nfft // S in (32, 64, 128, 256) else 0


def spectral_length(shape, K=None):
    """Samples per channel: K whole frames and hop - 1 more that belong to no frame."""
    K = shape["K"] if K is None else K
    hop = shape["n"] - shape["noverlap"]
    return (K - 1) * hop + shape["n"] + hop - 1


def spectral_units(case, K=None):
    """[units of every pass the call makes through its loop]: one entry per call of the loop (the multi-pass engine: per channel; streaming: per slice)."""
    sh = case.shape
    K = sh["K"] if K is None else K
    if case.loop.startswith("rocfft"):
        return [K * sh["nch"]]
    per = (lambda k: k) if is_complex(case.dtype) else (lambda k: (k + 1) // 2)
    if case.op == "stream":
        return [per(k) for k in sh["slices"]]
    return [per(K)] * sh["nch"]


# ---- overlap-save ------------------------------------------------------------------------------------------------------------------------------------
# shape: nb taps, nfft requested (0: the library's choice), mode, ncols, nblocks per column (of the EXECUTED block length; the last one 100 outputs short),
#        ld_pad (column strides nx + ld_pad, nout + ld_pad), range_from (first block of an mdsp_ols_exec_range call to the end of the column, or None)
# expect["geometry"] = (exec_nfft, exec_block_len, partitions, engine, rows) of mdsp_ols_geometry_for
def _ols(id, loop, dtype, nb, nfft, mode, ncols, nblocks, geometry, expect, engine=FUSED, create=None, launch=None, range_from=None, range_expect=None, ld_pad=3):
    shape = dict(nb=nb, nfft=nfft, mode=mode, ncols=ncols, nblocks=nblocks, ld_pad=ld_pad, range_from=range_from, engine=engine, nx_hint=1 << 28)
    expect = dict(expect, geometry=geometry, range=range_expect)
    return Case(id, loop, dtype, "ols", create or {}, launch or {}, shape, expect)


_LOG2N16 = {"MDSP_BIG_OLS_LOG2N": 16}      # blocks of 65536 points on natural-order spectra (run_ols): 512 KiB per transform, and two buffers of them
_NB = 16400                                # beyond four partitions of 8192 points (more than 16384 Float32 taps)
_G16 = (1 << 16, (1 << 16) - (_NB - 1), 1, FUSED, 0)
_G19 = (1 << 19, (1 << 19) - (_NB - 1), 1, FUSED, 64)
OLS = [
    # the fixed 64 MiB: 64-point blocks of a 12-tap filter are 520 bytes of intermediates each, 129055 per chunk.  Two columns of 129555 blocks:
    # 259110 units = 129055 + 129055 + 1000, and chunk 1 starts 500 blocks before the end of column 0
    _ols("rocfft-ols-float32", "rocfft_ols", F32, 12, 64, OLS_FILT, 2, 129555, (64, 53, 1, ROCFFT, 0), _e(3, 1000, spans=True, ref_chunks=3), engine=ROCFFT),
    # 8192-point ComplexF64 blocks are 128 KiB each (in place): 512 per chunk, 1030 blocks = 512 + 512 + 6
    _ols("rocfft-ols-complex128", "rocfft_ols", C64, 6001, 8192, OLS_CONV, 1, 1030, (8192, 2192, 1, ROCFFT, 0), _e(3, 6, ref_chunks=3), engine=ROCFFT),
    # run_ols at one transform per chunk (1 MiB over two buffers of 512 KiB); 5 real blocks are 3 units, the last one a single block; the range starts in chunk 1
    _ols("big-ols-float32-filt-c1", "big_ols", F32, _NB, 0, OLS_FILT, 1, 5, _G16, _e(3, 1, one_frame=True), create=_LOG2N16, launch=BIG1, range_from=2,
         range_expect=_e(2, 1, one_frame=True)),
    # two transforms per chunk at 2 MiB: 9 real blocks are 5 units = 2 + 2 + 1
    _ols("big-ols-float32-conv", "big_ols", F32, _NB, 0, OLS_CONV, 1, 9, _G16, _e(3, 1, one_frame=True), create=_LOG2N16, launch={"MDSP_BIG_CHUNK_MIB": 2}),
    _ols("big-ols-complex64-filt", "big_ols", C32, _NB, 0, OLS_FILT, 1, 5, _G16, _e(3, 1), create=_LOG2N16, launch={"MDSP_BIG_CHUNK_MIB": 2}),
    # 13 real blocks are 7 units = 2 + 2 + 2 + 1; the range from block 6 (unit 3, inside the whole call's chunk 1) runs units 3 .. 6 as 2 + 2: its seam falls
    # where the whole call has none
    _ols("big-ols-float32-filt-range", "big_ols", F32, _NB, 0, OLS_FILT, 1, 13, _G16, _e(4, 1, one_frame=True), create=_LOG2N16, launch={"MDSP_BIG_CHUNK_MIB": 2},
         range_from=6, range_expect=_e(2, 2, one_frame=True)),
    # run_ols_rows: the default form for this filter, 64 rows of 8192 points, 4 MiB per transform
    _ols("big-ols-rows-float32-filt-c1", "big_ols_rows", F32, _NB, 0, OLS_FILT, 1, 5, _G19, _e(3, 1, one_frame=True), launch={"MDSP_BIG_CHUNK_MIB": 4}, range_from=2,
         range_expect=_e(2, 1, one_frame=True)),
    _ols("big-ols-rows-float32-conv", "big_ols_rows", F32, _NB, 0, OLS_CONV, 1, 9, _G19, _e(3, 1, one_frame=True), launch={"MDSP_BIG_CHUNK_MIB": 8}),
    _ols("big-ols-rows-complex64-filt", "big_ols_rows", C32, _NB, 0, OLS_FILT, 1, 5, _G19, _e(3, 1), launch={"MDSP_BIG_CHUNK_MIB": 8}),
]


def ols_sizes(case):
    """(nx, nout) per column: nblocks blocks of the executed length, the last one 100 outputs short (half a block where blocks are shorter than 200)."""
    sh, L = case.shape, case.expect["geometry"][1]
    nout = sh["nblocks"] * L - min(100, L // 2)
    return (nout - (sh["nb"] - 1), nout) if sh["mode"] == OLS_CONV else (nout, nout)


def ols_units(case, g0=0):
    """(units the loop walks from block g0 to the end, units the chunk size is capped by)."""
    sh = case.shape
    nblocks = sh["nblocks"]
    if case.loop == "rocfft_ols":
        return nblocks * sh["ncols"] - g0, nblocks * sh["ncols"]
    u0, u1 = (g0, nblocks) if is_complex(case.dtype) else (g0 // 2, (nblocks + 1) // 2)
    return u1 - u0, u1 - u0


# ---- hilbert -----------------------------------------------------------------------------------------------------------------------------------------
# 1000-point Float32 columns are 16008 bytes of intermediates each (the samples, 501 bins, 1000 points of the full spectrum): 16768 per batch of 256 MiB,
# Float64 at 1001 points (an odd length): 8378.  Two batches and five columns; packed (ldx == n: the tail batch is staged through a cleared buffer) and strided (every batch is staged).
# The last case has more than 2^20 points per column: more than 4096 workgroups of 256 would cover it, so the kernels' grids are capped and stride.
def _hil(id, dtype, n, ncols, ld_pad, expect):
    return Case(id, "hilbert", dtype, "hilbert", {}, {}, dict(n=n, ncols=ncols, ld_pad=ld_pad), expect)


HILBERT = [
    _hil("hilbert-float32-packed", F32, 1000, 2 * 16768 + 5, 0, _e(3, 5, ref_chunks=3)),
    _hil("hilbert-float32-strided", F32, 1000, 2 * 16768 + 5, 5, _e(3, 5, ref_chunks=3)),
    _hil("hilbert-float64-packed", F64, 1001, 2 * 8378 + 5, 0, _e(3, 5, ref_chunks=3)),
    _hil("hilbert-float64-strided", F64, 1001, 2 * 8378 + 5, 5, _e(3, 5, ref_chunks=3)),
    _hil("hilbert-float32-long-columns", F32, 1050000, 2, 0, _e(1, 2, ref_chunks=1)),
]
HILBERT_GRID_CAP = 4096 * 256      # points of a column the capped grid covers in one step

CASES = SPECTRAL + OLS + HILBERT
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# plan re-use: one plan of each rocFFT kind run short, long and short again -- the cached batch size changes and the transforms are rebuilt both times.
# (case id, the short call: frames per channel / blocks per column / columns)
REUSE = (("rocfft-welch-float32-onesided", 5), ("rocfft-stft-float32-onesided-packed", 5), ("rocfft-ols-float32", 7), ("hilbert-float64-packed", 3))


def schedule(units, per_chunk, first=0):
    """[(first unit, count)] of a loop `for u0 = first; u0 < first + units; u0 += per_chunk`."""
    return [(u0, min(per_chunk, first + units - u0)) for u0 in range(first, first + units, per_chunk)]
