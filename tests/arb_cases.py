"""Case table of tests/test_gpu_arb_paths.py and tests/test_arb_reference_cpu.py: arbitrary-rate FIRFilter shapes on the boundaries of the
launch decisions of arbitrary_fir_kernel (csrc/fir_arb.hip, arb_geometry), each with the geometry mdsp_arb_kernel_geometry must report.  The
geometry was read off the predicates (256 compute units):

    taps_in_lds  2 tp nphi sizeof(R) <= 32 KiB
    nchg         min(4 if nch >= 3 else nch, MDSP_ARB_NCH), halved while records + taps + span nchg sizeof(A) > 44 KiB
    tile         MDSP_ARB_TILE (default 1024); with nchg = 1 halved while span sizeof(A) > 48 KiB
    span         (ceil(tile / rate) + tp + 7) & ~3; 0 (windows read from memory) if at tile 16 it still exceeds 48 KiB
    loop         gy = min(groups, max(1, ceil(8 CUs / tiles))) < groups: a workgroup restages for several channel groups

Row: (rate, nphi, hlen, taps dtype, signal dtype, nch, knobs, state, nout, geometry)
  knobs:    (name, value) pairs set through _lib.set_tunable for the case (T16 / T48: MDSP_ARB_TILE)
  state:    "fresh"; "delay" = setphase(timedelay()) first (a phase off the recurrence's grid, input_deficit > 1); "cont" = a stream that
            continues one of 37 + tp samples already filtered (checked like every other chunk)
  nout:     outputs of the main (last, largest) chunk, about: an int, or ("tiles", a, b) for 16 (a CUs + b) + 5 outputs, CUs from the device
  geometry: (nchg, tile, staged = span > 0, taps_in_lds, lds_bytes > 48 KiB, loop = gy < groups)

Rows of one (types, filter, rate, state) but different geometries form a family: their outputs are bit-identical, channel by channel.
"""
import ctypes as C
import functools
import zlib

import numpy as np

import arb_ref

T16 = (("MDSP_ARB_TILE", 16),)
T48 = (("MDSP_ARB_TILE", 48),)
N2 = (("MDSP_ARB_NCH", 2),)
N1 = (("MDSP_ARB_NCH", 1),)
S, M = 597, 2437                                 # 37 tiles of 16 (12 of 48) and 5 outputs more; two tiles of 1024 and 389
LOOP1, LOOP2 = ("tiles", 8, 3), ("tiles", 4, 1)  # tile 16: gy == 1 (three channel groups per workgroup), gy == 2 (row 0 takes groups 0 and 2)


def P(k):
    return (("MDSP_ARB_PRIO", k),)


CASES = [
    # --- Float32, 1.37, tp 6 (remainder batches 4 + 1), nphi 32: every way of cutting 1 .. 9 channels into groups and tiles
    (1.37, 32, 192, "f32", "f32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),            # f32 x 4: the 16-byte lane order
    (1.37, 32, 192, "f32", "f32", 4, T48, "fresh", S, (4, 48, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 4, (), "fresh", M, (4, 1024, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 4, T16 + N2, "fresh", S, (2, 16, True, True, False, False)),       # f32 x 2
    (1.37, 32, 192, "f32", "f32", 4, T16 + N1, "fresh", S, (1, 16, True, True, False, False)),       # f32 x 1
    (1.37, 32, 192, "f32", "f32", 1, T16, "fresh", S, (1, 16, True, True, False, False)),            # a channel alone
    (1.37, 32, 192, "f32", "f32", 9, T16, "fresh", LOOP1, (4, 16, True, True, False, True)),         # groups 0, 1, 2 in one workgroup (nc 4, 4, 1)
    (1.37, 32, 192, "f32", "f32", 9, T16, "fresh", LOOP2, (4, 16, True, True, False, True)),         # grid row 0: groups 0 and 2, row 1: group 1
    (1.37, 32, 192, "f32", "f32", 3, T16 + N1, "fresh", LOOP1, (1, 16, True, True, False, True)),
    (1.37, 32, 192, "f32", "f32", 3, T16 + N1, "fresh", LOOP2, (1, 16, True, True, False, True)),
    (1.37, 32, 192, "f32", "f32", 5, T16, "fresh", S, (4, 16, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 5, T16 + P(1), "fresh", S, (4, 16, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 5, T16 + P(2), "fresh", S, (4, 16, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 5, T16 + P(3), "fresh", S, (4, 16, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 2, T16, "delay", S, (2, 16, True, True, False, False)),
    (1.37, 32, 192, "f32", "f32", 2, T48 + N1, "delay", S, (1, 48, True, True, False, False)),
    # --- ComplexF64, 1.37: the 44 KiB rule halves four channels to two at the default tile (13056 + 3072 + 760 * 2 * 16 = 40448 bytes)
    (1.37, 32, 192, "f64", "c64", 4, (), "fresh", M, (2, 1024, True, True, False, False)),           # c64 x 2
    (1.37, 32, 192, "f64", "c64", 4, T16, "fresh", S, (4, 16, True, True, False, False)),            # c64 x 4
    (1.37, 32, 192, "f64", "c64", 1, T16, "fresh", S, (1, 16, True, True, False, False)),            # c64 x 1: 16 bytes
    (1.37, 32, 192, "f64", "c64", 2, T48, "fresh", S, (2, 48, True, True, False, False)),
    # --- Float64, 2.7, nphi 48, tp 10 (remainder 1 after one batch of 8)
    (2.7, 48, 437, "f64", "f64", 2, T16, "cont", S, (2, 16, True, True, False, False)),              # f64 x 2: 16 bytes
    (2.7, 48, 437, "f64", "f64", 4, T16, "cont", S, (4, 16, True, True, False, False)),              # f64 x 4
    (2.7, 48, 437, "f64", "f64", 3, T48, "cont", S, (4, 48, True, True, False, False)),              # three channels in a group of four
    (2.7, 48, 437, "f64", "f64", 1, (), "cont", M, (1, 1024, True, True, False, False)),
    # --- ComplexF32 with Float32 taps, 0.37, tp 17 (two batches of 8)
    (0.37, 32, 544, "f32", "c32", 2, T16, "fresh", S, (2, 16, True, True, False, False)),            # c32 x 2: 16 bytes
    (0.37, 32, 544, "f32", "c32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),            # c32 x 4
    (0.37, 32, 544, "f32", "c32", 5, T16 + N2, "fresh", S, (2, 16, True, True, False, False)),       # groups of 2, 2, 1
    (0.37, 32, 544, "f32", "c32", 1, T16, "fresh", S, (1, 16, True, True, False, False)),            # c32 x 1: 8 bytes
    (0.37, 32, 544, "f32", "c32", 2, (), "fresh", M, (1, 1024, True, True, False, False)),           # 44 KiB rule: 13056 + 4352 + 2792 * 2 * 8 is above it
    # --- the mixed arithmetic types
    (1.0, 32, 256, "f64", "f32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),             # tp 8: remainder 4 + 2 + 1
    (1.0, 32, 256, "f64", "f32", 3, T48, "delay", S, (4, 48, True, True, False, False)),
    (37.5, 7, 35, "f64", "c32", 2, T16, "fresh", S, (2, 16, True, True, False, False)),
    (0.5, 32, 320, "f32", "f64", 2, T16, "fresh", S, (2, 16, True, True, False, False)),             # delta integral: alpha identically 0
    (0.5, 32, 320, "f32", "f32", 4, T16, "delay", S, (4, 16, True, True, False, False)),
    (2.7, 20, 60, "f32", "c64", 3, T16, "cont", S, (4, 16, True, True, False, False)),               # tp 3: remainder 2
    # --- taps per phase 1 .. 16 with nphi 16 / 20 / 7 (run-time nphi) and the odd tap-table tail
    (1.37, 16, 16, "f32", "f32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),             # tp 1: no history
    (1.37, 16, 29, "f64", "f64", 2, T16, "fresh", S, (2, 16, True, True, False, False)),             # tp 2
    (2.7, 20, 77, "f32", "f32", 3, T16, "delay", S, (4, 16, True, True, False, False)),              # tp 4: remainder 2 + 1
    (37.5, 7, 35, "f32", "f32", 3, T16, "fresh", S, (4, 16, True, True, False, False)),              # tp 5, nphi 7: np = 35 is odd
    (37.5, 7, 35, "f32", "f32", 1, T48, "fresh", S, (1, 48, True, True, False, False)),
    (0.37, 16, 112, "f32", "f32", 2, T16, "cont", S, (2, 16, True, True, False, False)),             # tp 7: remainder 4 + 2
    (1.0, 16, 128, "f64", "c64", 1, T16, "delay", S, (1, 16, True, True, False, False)),             # tp 8
    (1.37, 16, 141, "f32", "f32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),            # tp 9: one batch of 8, no remainder
    (1.37, 16, 256, "f32", "c32", 3, T16, "fresh", S, (4, 16, True, True, False, False)),            # tp 16: 8 + 4 + 2 + 1
    (1.37, 1, 1, "f32", "f32", 1, T16, "fresh", S, (1, 16, True, True, False, False)),               # np = 1: a tap table of one 8-byte pair
    (1.37, 1, 1, "f32", "f32", 4, T16, "fresh", S, (4, 16, True, True, False, False)),
    # --- tap pairs in LDS / read from memory (32 KiB of pairs), dynamic LDS above 48 KiB (13056 + 32768 + 1156 * 4 = 50448 bytes)
    (1.0, 32, 4096, "f32", "f32", 1, (), "fresh", M, (1, 1024, True, True, True, False)),
    (1.0, 32, 4097, "f32", "f32", 1, (), "fresh", M, (1, 1024, True, False, False, False)),
    (1.37, 32, 4097, "f32", "f32", 4, T16, "fresh", S, (4, 16, True, False, False, False)),
    (1.37, 32, 2048, "f64", "f64", 2, T48, "fresh", S, (2, 48, True, True, False, False)),
    (1.37, 32, 2049, "f64", "f64", 2, T48, "fresh", S, (2, 48, True, False, False, False)),
    (0.0012, 32, 4097, "f32", "f32", 1, T16, "fresh", 72, (1, 16, False, False, False, False)),      # unstaged and taps from memory
    # --- very low rates: the unstaged path, the long staging loop, the automatic halving of the tile
    (0.0012, 16, 48, "f32", "f32", 1, T16, "fresh", 72, (1, 16, False, True, False, False)),
    (0.0012, 16, 48, "f32", "f32", 1, (), "fresh", 72, (1, 16, False, True, False, False)),          # 1024 halved down to 16
    (0.0012, 16, 48, "f32", "f32", 3, T16, "delay", 72, (1, 16, False, True, False, False)),         # the 44 KiB rule: 4 -> 1, then unstaged
    (0.0012, 16, 48, "f64", "c32", 2, T16, "fresh", 72, (1, 16, False, True, False, False)),
    (0.004, 16, 48, "f64", "c64", 2, T16, "fresh", 200, (1, 16, False, True, False, False)),
    (0.004, 16, 48, "f64", "f64", 1, T16, "fresh", 200, (1, 16, True, True, False, False)),          # staged: a span of 4008 samples
    (0.004, 16, 48, "f32", "c32", 2, T16, "fresh", 200, (1, 16, True, True, False, False)),          # 2 -> 1 by the 44 KiB rule, staged
    (0.04, 16, 48, "f32", "f32", 1, (), "fresh", 700, (1, 256, True, True, False, False)),           # 1024 -> 256: 6412 samples fit 48 KiB
]

NP_T = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}
GEOMETRY_FIELDS = ("nchg", "tile", "staged", "taps_in_lds", "lds_above_48k", "loop")


def case_id(c):
    rate, nphi, hlen, td, xd, nch, knobs, state, nout, _ = c
    kn = "-".join(f"{k.replace('MDSP_ARB_', '').lower()}{v}" for k, v in knobs)
    no = nout if isinstance(nout, int) else f"{nout[1]}cu{nout[2]}"
    return f"r{rate}_p{nphi}_h{hlen}_{td}_{xd}_c{nch}_{kn or 'default'}_{state}_n{no}"


def family(c):
    """Rows with the same family compute the same outputs, channel by channel, whatever their geometry."""
    rate, nphi, hlen, td, xd, nch, knobs, state, nout, _ = c
    return (rate, nphi, hlen, td, xd, state)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def taps(c):
    rate, nphi, hlen, td = c[:4]
    h = np.random.default_rng(_seed("h", rate, nphi, hlen)).standard_normal(hlen) / np.sqrt(max(1.0, hlen / nphi))
    return h.astype(NP_T[td])


def signal(c, n):
    """(nch, n) samples; channel k of a family is the same stream in every row, and a longer stream extends a shorter one."""
    xd, nch = c[4], c[5]
    x = np.empty((nch, n), dtype=NP_T[xd])
    for k in range(nch):
        v = np.random.default_rng(_seed("re", family(c), k)).standard_normal(n)
        if xd[0] == "c":
            v = v + 1j * np.random.default_rng(_seed("im", family(c), k)).standard_normal(n)
        x[k] = v.astype(NP_T[xd])
    return x


def initial_state(c):
    """(phi_acc, input_deficit, phi) before the first chunk; phi is what setphase gets (None: not called).  setphase! stream_filt.jl:231-239."""
    rate, nphi, hlen = c[:3]
    if c[7] != "delay":
        return 0.0, 1, None
    phi = (hlen - 1) / (2 * nphi)                                      # timedelay, :400-401
    whole = float(int(phi))
    return (phi - whole) * nphi, 1 + round(whole), phi


def target_nout(c, cu):
    nout = c[8]
    return nout if isinstance(nout, int) else 16 * (nout[1] * cu + nout[2]) + 5


@functools.lru_cache(maxsize=None)
def plan(c, cu=256):
    """(n, cuts, nouts): the stream length, the chunk boundaries {0, [37 + tp,] +1, an odd point near a third, tp - 2 samples more, n} and the outputs
    of every chunk, from the reference trajectory.  n is the smallest length (from 1.5 target / rate on) whose last chunk -- the main one, the one the
    row's geometry is about -- has at least the target number of outputs and not a multiple of 16 (a partial last tile and anchor block)."""
    rate, nphi, hlen = c[:3]
    tp = -(-hlen // nphi)
    target = target_nout(c, cu)
    acc0, def0, _ = initial_state(c)
    pre = 37 + tp if c[7] == "cont" else 0
    n = pre + int(1.5 * target / rate) + 2
    while True:
        odd = pre + (((n - pre) // 3) | 1)
        cuts = [0] + ([pre] if pre else []) + [pre + 1, odd, odd + max(tp - 2, 0), n]
        cuts = [int(b) for b in np.maximum.accumulate(np.minimum(cuts, n))]    # (a short stream: chunks of no samples stay in, they are legal)
        acc, dfc, nouts = acc0, def0, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            xs, _, acc, dfc = arb_ref.trajectory(acc, dfc, rate, nphi, b - a)
            nouts.append(len(xs))
        if nouts[-1] >= target and nouts[-1] % 16:
            return n, cuts, nouts
        n += 1


def geometry(c, nout, cu):
    """mdsp_arb_kernel_geometry under the row's knobs: (tile, span, nchg, groups, tiles, gy, taps_in_lds, lds_bytes)."""
    from dsp_jl_amd import _lib
    rate, nphi, hlen, td, xd, nch, knobs = c[:7]
    lt = {"f32": _lib.F32, "f64": _lib.F64, "c32": _lib.C32, "c64": _lib.C64}
    out = (C.c_int64 * 8)()
    try:
        for k, v in knobs:
            _lib.set_tunable(k, v)
        _lib.check(_lib.lib().mdsp_arb_kernel_geometry(-(-hlen // nphi), nphi, float(rate), lt[td], lt[xd], nch, nout, cu, out))
    finally:
        for k, v in knobs:
            _lib.set_tunable(k, None)
    return tuple(out)


def reported(g):
    """The row form (nchg, tile, staged, taps_in_lds, lds above 48 KiB, loop) of a geometry."""
    tile, span, nchg, groups, tiles, gy, tlds, lds = g
    return (nchg, tile, span > 0, bool(tlds), lds > 48 * 1024, gy < groups)
