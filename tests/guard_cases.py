"""Case tables of the guard-band tests (tests/test_gpu_guard_ols.py, tests/test_gpu_guard_spectral.py): which plans they run, and what each is expected to
execute.  No device: tests/test_guard_bands_cpu.py holds the tables to the library's own host arithmetic (mdsp_ols_geometry_for / _tile_for / _stream_for,
mdsp_spectral_route_for against tests/spectral_route_cases.py), so that a kernel form cannot drop out of the guard tests without a failure."""
from collections import namedtuple

import numpy as np

F32, F64, C32, C64 = 0, 1, 2, 3
NP_DTYPE = {F32: np.float32, F64: np.float64, C32: np.complex64, C64: np.complex128}
AUTO, FUSED, ROCFFT = 0, 1, 2

# ---- overlap-save ------------------------------------------------------------------------------------------------------------------------------------
# create: knobs set while the plan is made; launch: knobs set around the calls.  lengths: "all" = L // 2, L, L + 1, 2 L, 3 L + 3; "rows" = L // 2, L + 1,
# 2 L + 17; "short" = L // 2, L + 1 (L: tile).  expect = (exec_nfft, partitions, rows, engine, tile, lead); streaming: what mdsp_ols_stream_for answers
# under the launch knobs (0 / 1; the kernel whose loads and stores bypass the caches).  nfft is the REQUESTED length: long filters are re-blocked.
OlsForm = namedtuple("OlsForm", "id dtype nb nfft engine create launch ncols lengths expect streaming")


def _f(id, dtype, nb, nfft, expect, engine=FUSED, create=None, launch=None, ncols=3, lengths="all", streaming=0):
    return OlsForm(id, dtype, nb, nfft, engine, create or {}, launch or {}, ncols, lengths, expect, streaming)


OLS_FORMS = [
    _f("f32-64-256", F32, 64, 256, (256, 1, 0, FUSED, 193, 63)),
    _f("f32-200-1024", F32, 200, 1024, (1024, 1, 0, FUSED, 825, 199)),
    _f("f32-256-2048-untiled", F32, 256, 2048, (2048, 1, 0, FUSED, 1793, 255), create={"MDSP_OLS_TILE": 0}),
] + [
    _f(f"f32-{nb}-2048-tiled-stream{s}", F32, nb, 2048, (2048, 1, 0, FUSED, 1792, 256), launch={"MDSP_OLS_STREAM": s}, streaming=s // 2)
    for nb in (249, 256, 257) for s in (0, 2)
] + [
    # a mixed-radix length: no fused overlap-save kernel takes it (fused_supported: powers of two), AUTO runs the rocFFT engine at that very length
    _f("f32-100-1000-mixed-radix", F32, 100, 1000, (1000, 1, 0, ROCFFT, 901, 99), engine=AUTO),
    _f("f32-1500-reblocked", F32, 1500, 16384, (8192, 1, 0, FUSED, 6693, 1499)),
    _f("f32-5120-3-partitions", F32, 5120, 16384, (4096, 3, 0, FUSED, 2048, 5119)),
    _f("f32-7000-4-partitions", F32, 7000, 16384, (4096, 4, 0, FUSED, 2048, 6999)),
    _f("f32-20001-rows64", F32, 20001, 65536, (1 << 19, 1, 64, FUSED, (1 << 19) - 20000, 20000), lengths="rows"),
    _f("f32-150000-rows256", F32, 150000, 1 << 19, (1 << 21, 1, 256, FUSED, (1 << 21) - 149999, 149999), ncols=1, lengths="short"),
    _f("f32-40000-three-pass", F32, 40000, 1 << 17, (1 << 20, 1, 0, FUSED, (1 << 20) - 39999, 39999), create={"MDSP_BIG_OLS_ROWS": 0}, ncols=2, lengths="short"),
    _f("f64-200-1024", F64, 200, 1024, (1024, 1, 0, FUSED, 825, 199)),
    _f("f64-5120-3-partitions", F64, 5120, 16384, (4096, 3, 0, FUSED, 2048, 5119)),
    _f("f64-20001-rows64", F64, 20001, 65536, (1 << 18, 1, 64, FUSED, (1 << 18) - 20000, 20000), lengths="rows"),
    _f("c32-200-1024", C32, 200, 1024, (1024, 1, 0, FUSED, 825, 199)),
    _f("c64-200-1024", C64, 200, 1024, (1024, 1, 0, FUSED, 825, 199)),
    _f("c32-20001-multipass", C32, 20001, 65536, (1 << 19, 1, 64, FUSED, (1 << 19) - 20000, 20000), lengths="rows"),
    _f("f32-200-1024-rocfft", F32, 200, 1024, (1024, 1, 0, ROCFFT, 825, 199), engine=ROCFFT),
    _f("c32-200-1024-rocfft", C32, 200, 1024, (1024, 1, 0, ROCFFT, 825, 199), engine=ROCFFT),
]
OLS_BY_ID = {f.id: f for f in OLS_FORMS}
# block ranges (mdsp_ols_exec_range): the tiled plan (its ranges run the untiled blocks) and the 3-partition plan
OLS_RANGE_FORMS = ("f32-256-2048-tiled-stream0", "f32-5120-3-partitions")


def ols_lengths(form):
    """The signal lengths of a form; L is the executed tile (== block on every untiled plan)."""
    L = form.expect[4]
    return {"all": (L // 2, L, L + 1, 2 * L, 3 * L + 3), "rows": (L // 2, L + 1, 2 * L + 17), "short": (L // 2, L + 1)}[form.lengths]


def ols_nouts(form, nx, conv):
    """FILT: nx and a length that truncates inside a block (clamped at 0 where the signal is shorter than that); CONV: the full convolution and nx + 1."""
    L = form.expect[4]
    return (nx + form.nb - 1, nx + 1) if conv else (nx, max(0, nx - 1 - L // 2))


# ---- Welch / STFT / multitaper -----------------------------------------------------------------------------------------------------------------------
KIND_WELCH, KIND_STFT = 0, 1
POW2_ROUTE = "1"                  # MDSP_ROUTE_POW2: every size is a kernel of its own (4096 Float32 Welch is hand-written assembly)
ROCFFT_NFFT = 1024                # the one size run under engine ROCFFT


def spectral_cases(kind, dtype):
    """[(engine, nfft, route character)] from the committed table of tests/spectral_route_cases.py: under engine AUTO the smallest nfft >= 8 of every route
    the table holds for (kind, dtype) and EVERY size of the power-of-two register route; under engine FUSED the same, less the sizes whose route AUTO takes
    too (the same kernel: the AUTO case runs it); one size under engine ROCFFT."""
    import spectral_route_cases as src
    table = src.expected_default()
    picks = {}
    for engine in (AUTO, FUSED):
        first = set()
        picks[engine] = []
        for n, c in zip(src.SIZES, table[(kind, dtype, engine)][0]):
            if n < 8 or c == "-" or (c != POW2_ROUTE and c in first):
                continue
            first.add(c)
            picks[engine].append((n, c))
    auto_at = dict(zip(src.SIZES, table[(kind, dtype, AUTO)][0]))
    cases = [(AUTO, n, c) for n, c in picks[AUTO]] + [(FUSED, n, c) for n, c in picks[FUSED] if auto_at[n] != c]
    return cases + [(ROCFFT, ROCFFT_NFFT, "0")]


def spectral_shapes(nfft):
    """(n, noverlap, hop, len) per size: a frame that fills the transform and one whose tail is zero padding; three whole frames -- an odd count: the
    last unit of a real signal has no second frame -- and hop - 1 samples that belong to no frame."""
    out = []
    for n in (nfft, nfft - nfft // 4 - 1):
        nov = n // 2
        hop = n - nov
        out.append((n, nov, hop, n + 2 * hop + hop - 1))
    return out


# multitaper (kind 1 routes): one power-of-two size, one of the run-time-schedule kernel, one of the multi-pass engine, per dtype from the same table
def mt_sizes(dtype):
    by_route = {c: n for e, n, c in reversed(spectral_cases(KIND_STFT, dtype)) if e == AUTO}
    return [(1024, POW2_ROUTE), (by_route["3"], "3"), (by_route["a"], "a")]
