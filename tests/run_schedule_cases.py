"""Host arithmetic of the persistent kernels' unit schedule, and the case tables of tests/test_gpu_run_schedules.py.  Pure Python: no GPU, no library.

Every fused spectral and overlap-save kernel is persistent: a SLOT (one transform's worth of threads) walks RUNS of `run_len` consecutive units.  The
host sizes the grid as min(work, CUs x workgroups per CU), so at the shapes the rest of the suite uses a slot gets at most one unit, run_len is 1,
and everything that only happens between two consecutive units of a run never executes: the ComplexF32 register carry (the `f == held + 1` branch of
stft_fused_kernel / welch_fused_kernel), the walk itself (walk(), unit_cur(), dead units, a partial last run, idle slots, a second run per slot) and
the prefetching form of ols_fused_kernel.  With MDSP_WG_PER_CU=1 and two channels the grid is small enough that a few hundred to a few thousand
units give every slot a run of three; this module works out how many, from the same arithmetic the host uses.

What is mirrored (dsp.jl_amd/csrc):
    geometry   spectral_op.h `template <typename R, int N> struct Geo` (EMAX / E / T / G), welch.hip welch_launch_n (the half-frame kernels' EH / GH and the real
               Float32 nfft 4096 launch with 16 elements per thread), ols.hip launch_fused_n (EMAX / E / T / G, one transform per workgroup for real
               Float32 nfft 2048), common.h slots_per_workgroup
    schedule   spectral_op.h set_schedule, ols.hip launch_fused_geo (the same two lines)
    slots      spectral_op.h grid_for (the channels SHARE the resident workgroups: grid.y = channels), ols.hip launch_fused_geo (units span the columns)
    carry_shift  stft.hip stft_launch_n / welch.hip welch_launch_n: `shift = (n == N && hop % T == 0 && hop / T < E) ? hop / T : 0` and the instantiated SHIFTs

tests/test_run_schedule_cases_cpu.py holds these tables to the properties the GPU tests rely on, for several CU counts: a change of a geometry that
would quietly turn a case back into run_len == 1, or a SHIFT case into the generic kernel, fails there.
"""
import numpy as np

F32, F64, C32, C64 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)

NCH = 2            # channels of every spectral case (different seeds)
OLS_NCOLS = 3      # columns of every overlap-save case
CU_COUNTS = (64, 104, 256, 304)   # the CPU test's CU counts (the GPU tests ask the device)


def _cdiv(a, b):
    return -(-a // b)


def _is_double(dtype):
    return np.dtype(dtype) in (F64, C64)


def _is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def slots_per_workgroup(T):
    """common.h: `T >= 128 ? 1 : 256 / T` (one transform per workgroup wherever its waves meet at a barrier)."""
    return 1 if T >= 128 else 256 // T


def geometry(kind, dtype, nfft):
    """(E, T, G): elements per thread, threads per transform, transforms (slots) per workgroup.

    kind  "stft"        stft_fused_kernel, stft_pair_kernel: Geo<R, N> (stft.hip stft_launch_n)
          "welch"       welch_fused_kernel: Geo<R, N>, except real Float32 nfft 4096, launched with E = 16, G = 1 (welch_launch_n, "the headline shape
                        off the half-frame path")
          "welch_half"  welch_half_kernel / welch_half3_kernel (real, n == nfft, hop == n/2): EH = 16 for Float32 nfft >= 2048, else Geo's E
          "ols"         ols_fused_kernel (ols.hip launch_fused_n)
    """
    dtype = np.dtype(dtype)
    dbl = _is_double(dtype)
    if kind == "ols":
        emax = 16 if (not dbl and nfft >= 1024) else 8                  # launch_fused_n: `EMAX = (!DBL && N >= 1024) ? 16 : 8`
        E = min(nfft // 64, emax)
        T = nfft // E
        G = slots_per_workgroup(T)
        if nfft == 2048 and dtype == F32:                               # `if constexpr (N == 2048 && !CPLX && !DBL)`: <R, N, 16, 1, ...>
            E, T, G = 16, 128, 1
        return E, T, G
    emax = 16 if (nfft == 1024 and not dbl) else 8                      # Geo: `EMAX = (N == 1024 && !DBL) ? MDSP_GEO_E1024 : 8`
    E = min(nfft // 64, emax)
    if kind == "welch" and dtype == F32 and nfft == 4096:               # welch_run_fused<R, N, 16, 1, 1, 4, CPLX, 1, false>
        E = 16
    elif kind == "welch_half":
        if _is_complex(dtype):
            raise ValueError("the half-frame kernels take real signals")
        if nfft >= 2048 and not dbl:                                    # `EH = (N >= 2048 && sizeof(R) == 4) ? 16 : Gm::E`
            E = 16
    elif kind not in ("stft", "welch"):
        raise ValueError(kind)
    T = nfft // E
    return E, T, slots_per_workgroup(T)


def schedule(nunits, slots, runs=1):
    """(run_len, niter) as set_schedule (spectral_op.h) and launch_fused_geo (ols.hip) write them:
        run_len = max(1, cdiv(nunits, nslots * runs));  niter = cdiv(cdiv(nunits, run_len), nslots) * run_len
    Slot s walks the runs s, s + nslots, s + 2 nslots, ...; run g covers the units [g run_len, (g + 1) run_len)."""
    run_len = max(1, _cdiv(nunits, slots * runs))
    niter = _cdiv(_cdiv(nunits, run_len), slots) * run_len
    return run_len, niter


def slots(cu, nch, G, kind):
    """Transform slots of a launch under MDSP_WG_PER_CU=1 once the work exceeds them.  Spectral kernels (grid_for): the channels share the resident
    workgroups, max(1, cu // nch) * G per channel.  Overlap-save (launch_fused_geo): the units span the columns, cu * G in all."""
    if kind == "ols":
        return cu * G
    return max(1, cu // nch) * G


def units_for(nslots):
    """3 nslots - 4 units: with one run per slot run_len = 3, the last run holds 2 units and one slot idles; with MDSP_RUNS_PER_SLOT=2 run_len = 2
    and about half of the slots walk a second run, so that a register carry has to restart at a run boundary."""
    return 3 * nslots - 4


def ols_units_per_col(nslots, ncols=OLS_NCOLS):
    """Units per column of an overlap-save case.  The kernel's units are numbered through the columns, so their total is a multiple of the column
    count, which units_for() never is with three columns (3 s - 4 = 2 mod 3), and every multiple of three that gives run_len = 3 fills its last run.
    The smallest column at or above units_for(nslots) / ncols is taken for which the default schedule still has run_len >= 3, a partial last run and
    an idle slot: three columns of nslots + 1 units, run_len = 4, unless that total is a multiple of four."""
    upc = _cdiv(units_for(nslots), ncols)
    while True:
        total = upc * ncols
        run_len, _ = schedule(total, nslots, 1)
        if run_len >= 3 and total % run_len != 0 and _cdiv(total, run_len) < nslots:
            return upc
        upc += 1


def runs_of_slot(nunits, nslots, runs, s):
    """[(first unit, one past the last unit)] of slot s, in the order it walks them."""
    run_len, niter = schedule(nunits, nslots, runs)
    out = []
    for g in range(s, _cdiv(nunits, run_len), nslots):
        out.append((g * run_len, min(nunits, (g + 1) * run_len)))
    assert len(out) * run_len <= niter
    return out


# the SHIFTs stft_launch_n / welch_launch_n instantiate (stft.hip, welch.hip): 1, 2, 4 where E > 4, and for the STFT 8 where E > 8 (nfft 1024)
def _instantiated_shifts(op, E):
    if E <= 4:
        return ()
    if op == "stft":
        return (1, 2, 4, 8) if E > 8 else (1, 2, 4)
    if op == "welch":
        return (1, 2, 4)
    raise ValueError(op)


def carry_shift(op, dtype, nfft, n, hop):
    """SHIFT of the register-carry instantiation a (dtype, nfft, n, hop) STFT (op "stft") or Welch (op "welch") call is dispatched to; 0: the kernel
    without the carry.  The host's condition: ComplexF32, E > 4, n == nfft, hop % T == 0, hop // T == SHIFT < E, SHIFT instantiated."""
    if np.dtype(dtype) != C32:
        return 0
    E, T, _ = geometry(op, dtype, nfft)
    if n != nfft or hop % T != 0 or hop // T >= E:
        return 0
    return hop // T if hop // T in _instantiated_shifts(op, E) else 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------------------
CARRY_NFFT = (512, 1024, 2048, 4096, 8192)

# (nfft, SHIFT): ComplexF32, n = nfft, hop = SHIFT * T
STFT_SHIFT_CASES = tuple((nfft, sh) for nfft in CARRY_NFFT for sh in (1, 2, 4)) + ((1024, 8),)
WELCH_SHIFT_CASES = tuple((nfft, sh) for nfft in CARRY_NFFT for sh in (1, 2, 4))


def shift_case(op, nfft, shift):
    """(dtype, nfft, n, hop) of a SHIFT case."""
    _, T, _ = geometry(op, C32, nfft)
    return C32, nfft, nfft, shift * T


def control_cases(op):
    """(id, dtype, nfft, n, hop): the dispatch edge.  None of them may take a carry instantiation; all run with the same number of frames."""
    out = []
    for nfft in (512, 1024, 2048):
        E, T, _ = geometry(op, C32, nfft)
        out.append((f"{nfft}-no-overlap", C32, nfft, nfft, E * T))                 # SHIFT would equal E
        out.append((f"{nfft}-hop-1.5T", C32, nfft, nfft, T + T // 2))              # hop is no multiple of T
        out.append((f"{nfft}-n-short", C32, nfft, nfft - T, T))                    # n != nfft
    E, T, _ = geometry(op, C32, 256)
    out.append(("256-E4", C32, 256, 256, T))                                       # E = 4: no carry instantiation at all
    out.append(("1024-ComplexF64", C64, 1024, 1024, 256))                          # the carry is wired for ComplexF32 only
    if op == "welch":
        out.append(("1024-shift8", C32, 1024, 1024, 8 * geometry(op, C32, 1024)[1]))   # SHIFT 8 exists for the STFT only
    return tuple(out)


# real signals, run walk: (dtype, nfft)
REAL_CASES = tuple((F32, nfft) for nfft in (256, 512, 1024, 2048, 4096, 8192)) + tuple((F64, nfft) for nfft in (256, 512, 1024, 2048, 4096))


def real_stft_forms(nfft):
    """(id, n, hop, onesided) of the stft_pair_kernel cases of one nfft: whole frames at 50 % overlap one-sided, a zero tail two-sided."""
    n2 = nfft - 3
    return (("onesided", nfft, nfft // 2, True), ("twosided-ztail", n2, n2 // 3, False))


def real_welch_forms(nfft):
    """(id, kind, n, hop): welch_half_kernel (hop = n/2; Float32 nfft 4096: welch_half3_kernel) and welch_fused_kernel."""
    n3 = nfft - 3
    return (("half", "welch_half", nfft, nfft // 2), ("quarter", "welch", nfft, nfft // 4), ("ztail", "welch", n3, n3 // 3))


def real_frames(nslots):
    """Frames of a real case: units are frame PAIRS, and K is odd so that the last unit carries one frame."""
    return 2 * units_for(nslots) - 1


# overlap-save: (dtype, nfft); nb = nfft // 8 + 1 taps, OLS_NCOLS columns
OLS_CASES = (tuple((F32, nfft) for nfft in (256, 512, 1024, 2048, 4096, 8192)) + tuple((F64, nfft) for nfft in (256, 512, 1024, 2048, 4096))
             + tuple((C32, nfft) for nfft in (256, 512, 1024, 2048, 4096, 8192)) + tuple((C64, nfft) for nfft in (256, 512, 1024, 2048, 4096)))
OLS_RUNS = 3       # the MDSP_RUNS_PER_SLOT of the third overlap-save setting


def ols_taps(nfft):
    return nfft // 8 + 1


def ols_shape(dtype, nfft, cu):
    """(nb, L, blocks per column, column length nx, units per column, slots).  A unit is two blocks (real) or one (complex); real columns have an odd
    block count, so every column ends on a unit with one block; the last block of a column is partial."""
    _, _, G = geometry("ols", dtype, nfft)
    ns = slots(cu, OLS_NCOLS, G, "ols")
    upc = ols_units_per_col(ns)
    nb = ols_taps(nfft)
    L = nfft - nb + 1
    nblocks = upc if _is_complex(dtype) else 2 * upc - 1
    nx = (nblocks - 1) * L + L // 2 + 3
    return nb, L, nblocks, nx, upc, ns


def case_id(*parts):
    return "-".join(np.dtype(p).name if isinstance(p, (np.dtype, type)) else str(p) for p in parts)
