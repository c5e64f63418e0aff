"""CPU checks of tests/arb_ref.py and tests/arb_cases.py, the reference and the case table of the arbitrary-rate GPU sweep
(tests/test_gpu_arb_paths.py):

  (a) the reference agrees with the Float64 oracle (oracle.stream_filt.FIRFilter(h, rate, nphi).filt) in outputs, count and state after every
      chunk, for every filter shape of the table;
  (b) a NumPy emulation of the kernel's arithmetic (the fma chain in tap order in the arithmetic's precision, the combination in Float64, one
      rounding) passes the bound |y - ref| <= 2 (tp + 2) u absdot + 4 u_min on every row;
  (c) six subtly wrong kernels each fail it on at least one row, which the test names: the bound is not vacuous;
  (d) mdsp_arb_kernel_geometry (pure host arithmetic at 256 compute units) reports every row's expected geometry;
  (e) the staged span covers the windows of every tile of every row, so `staged` in the kernel is `span > 0`.
"""
import ctypes as C

import numpy as np
import pytest

import arb_cases as ac
from arb_cases import CASES, case_id, geometry, reported
from arb_ref import LD, accumulation_unit, arb_ref, excess, trajectory

IDS = [case_id(c) for c in CASES]
SHAPES = {}
for _c in CASES:
    SHAPES.setdefault((_c[0], _c[1], _c[2]), _c)                       # the first row of every (rate, nphi, hlen)


def _wide(x):
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


# --- (a) -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES), ids=[f"r{s[0]}_p{s[1]}_h{s[2]}" for s in SHAPES])
def test_reference_equals_the_oracle(shape):
    from oracle import stream_filt as osf
    c = SHAPES[shape]
    rate, nphi, hlen, td, xd = c[:5]
    tp = -(-hlen // nphi)
    h = ac.taps(c)
    n = int(160 / rate) + tp + 40                                      # about 160 outputs: the oracle is a Python loop per output
    x = ac.signal(c, n)[0]
    of = osf.FIRFilter(h, float(rate), nphi)                           # dh = diff(h) in eltype(h) (stream_filt.jl:107) ...
    of.h, of.pfb, of.dpfb = h.astype(np.float64), of.pfb.astype(np.float64), of.dpfb.astype(np.float64)   # ... the dot products in Float64
    acc, dfc, phi = ac.initial_state(c)
    if phi is not None:
        of.setphase(phi)
    assert (of.phi_acc, of.input_deficit) == (acc, dfc)
    hist = None
    odd = (n // 3) | 1
    cuts = [0, 1, odd, odd + max(tp - 2, 0), odd + max(tp - 2, 0), n]  # (with a chunk of no samples)
    total = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        yo = of.filt(_wide(x[a:b]))
        y, ad, (acc, dfc, hist) = arb_ref(h, rate, nphi, x[a:b], acc, dfc, hist)
        assert y.shape == yo.shape, (a, b)
        assert (acc, dfc) == (of.phi_acc, of.input_deficit), (a, b)
        assert np.array_equal(_wide(hist), of.history), (a, b)
        total += y.size
        if y.size:
            # the oracle's Float64 dot products and combination against the long-double ones: (tp + 2) 2^-53 absdot element-wise
            worst, _ = excess(yo, y, ad, tp, 2.0 ** -53 / 2, 0.0)
            assert worst <= 1.0, (shape, a, b, worst)
    assert total >= 100


def test_reference_state_of_short_chunks():
    # a chunk shorter than the deficit produces nothing and only lowers the deficit (stream_filt.jl:586-590)
    h = np.arange(1.0, 50.0)
    y, ad, (acc, dfc, hist) = arb_ref(h, 1.37, 7, np.ones(2), phi_acc=3.25, input_deficit=5)
    assert y.size == 0 and ad.size == 0 and (acc, dfc) == (3.25, 3) and np.array_equal(hist, [0.0] * 4 + [1.0, 1.0])
    assert arb_ref(h, 1.37, 7, np.ones(0), 3.25, 5)[2][:2] == (3.25, 5)


# --- the emulated kernel and its mutants -------------------------------------------------------------------------------------------------------

def _fma(a, b, c, R):
    """fma(a, b, c) in precision R on arrays: Float32 through Float64 (the product is exact there), Float64 through long double."""
    if R == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


MUTANTS = ("last remainder batch skipped", "record read without the pad slot", "one tile's window a sample late", "two channels of a group swapped",
           "restaged with the first group's channels", "tap-table tail pair left unset")


def emulate(c, x, acc, dfc, hist, mutant=None):
    """One chunk of the row's kernel in NumPy: per output and channel lo = p_0 z_0, lo = fma(z_k, p_k, lo), k = 1 .. tp - 1 in the arithmetic's
    precision R (up likewise with the derivative bank), y = R(fma(up, alpha, lo) in Float64).  `mutant` makes it subtly wrong the way a kernel bug
    would, using the row's tile and channel grouping.  Returns None when the mutant does not apply to the row."""
    rate, nphi, hlen, td, xd, nch, knobs, state, nout_class, geo = c
    nchg, tile = geo[0], geo[1]
    h = ac.taps(c)
    dbl = td == "f64" or xd in ("f64", "c64")
    R = np.float64 if dbl else np.float32
    tp = -(-hlen // nphi)
    from oracle.stream_filt import taps2pfb
    pfb = taps2pfb(h, nphi).astype(R)
    dpfb = taps2pfb(np.concatenate([np.diff(h), np.zeros(1, dtype=h.dtype)]).astype(h.dtype), nphi).astype(R)
    hl = tp - 1
    if hist is None:
        hist = np.zeros((nch, hl), dtype=x.dtype)
    z = np.concatenate([hist, x], axis=1)
    xs, accs, _, _ = trajectory(acc, dfc, rate, nphi, x.shape[1])
    nout = len(xs)
    if nout == 0:
        return np.zeros((nch, 0), dtype=z.dtype)
    m = np.arange(nout)
    j = m % tile
    start = xs - 1
    chan = np.arange(nch)
    ntap = tp
    if mutant == MUTANTS[0]:
        if (tp - 1) % 2 == 0:
            return None
        ntap = tp - 1
    elif mutant == MUTANTS[1]:
        if tile <= 16:                                                 # (outputs 0 .. 15 of a tile have slot j either way)
            return None
        # records live at slot j + j / 16; reading slot j finds the record of j' with j' + j' / 16 == j, or a pad slot (never written: 0 here)
        jp = j - j // 17
        pad = j % 17 == 16
        accs = np.where(pad, 0.0, accs[np.minimum(m - j + jp, nout - 1)])
    elif mutant == MUTANTS[2]:
        t = 1 if nout > tile else 0
        start = start + ((m // tile) == t)
        z = np.concatenate([z, np.zeros((nch, 1), dtype=z.dtype)], axis=1)
    elif mutant == MUTANTS[3]:
        if nchg < 2 or nch < 2:
            return None
        chan[[0, 1]] = chan[[1, 0]]
    elif mutant == MUTANTS[4]:
        if not geo[5]:
            return None
        groups = -(-nch // nchg)
        gy = 1 if nout_class == ac.LOOP1 else 2
        for g in range(groups):
            first = g % gy
            if g != first:                                             # a later group of the same workgroup: the first group's samples again
                for k in range(min(nchg, nch - g * nchg)):
                    chan[g * nchg + k] = first * nchg + k
    elif mutant == MUTANTS[5]:
        if R != np.float32 or (tp * nphi) % 2 == 0 or not geo[3]:
            return None
        pfb, dpfb = pfb.copy(), dpfb.copy()
        pfb[tp - 1, nphi - 1] = 0                                      # pair np - 1 of the LDS copy: never written
        dpfb[tp - 1, nphi - 1] = 0
    col = np.floor(accs).astype(np.int64)
    alpha = accs - np.floor(accs)
    parts = [z.real, z.imag] if np.iscomplexobj(z) else [z]
    out = []
    for zp in parts:
        zr = zp[chan].astype(R)
        lo = (pfb[0, col] * zr[:, start]).astype(R)
        up = (dpfb[0, col] * zr[:, start]).astype(R)
        for k in range(1, ntap):
            zk = zr[:, start + k]
            lo = _fma(zk, np.broadcast_to(pfb[k, col], zk.shape), lo, R)
            up = _fma(zk, np.broadcast_to(dpfb[k, col], zk.shape), up, R)
        out.append((up.astype(LD) * alpha.astype(LD) + lo.astype(LD)).astype(np.float64).astype(R))
    return out[0] + 1j * out[1] if len(out) == 2 else out[0]


def _run(c, mutant=None):
    """The row's stream through the reference and the (mutated) emulation, chunk by chunk: the largest excess over the bound, and the margin."""
    rate, nphi, hlen, td, xd = c[:5]
    tp = -(-hlen // nphi)
    n, cuts, nouts = ac.plan(c)
    x = ac.signal(c, n)
    h = ac.taps(c)
    u, umin = accumulation_unit(h.dtype, x.dtype)
    acc, dfc, _ = ac.initial_state(c)
    hist = None
    worst, ratio = 0.0, 0.0
    for (a, b), no in zip(zip(cuts[:-1], cuts[1:]), nouts):
        y = emulate(c, x[:, a:b], acc, dfc, hist, mutant)
        if y is None:
            return None, None
        ref, ad, (acc, dfc, hist) = arb_ref(h, rate, nphi, x[:, a:b], acc, dfc, hist)
        assert ref.shape[1] == no
        w, r = excess(y, ref, ad, tp, u, umin)
        worst, ratio = max(worst, w), max(ratio, r)
    return worst, ratio


@pytest.fixture(scope="module")
def correct():
    return {}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_emulated_kernel_is_within_the_bound(c, correct):
    worst, ratio = _run(c)
    tp = -(-c[2] // c[1])
    print(f"\nemulated {case_id(c)}: {worst:.3f} of the bound, max|y-ref|/(u absdot)={ratio:.3f} of {2 * (tp + 2)}")
    correct[case_id(c)] = worst
    assert worst <= 1.0


# the rows a mutant is tried on: the smallest of every kind it can apply to (the whole table would only repeat them)
def _mutant_rows(mutant):
    small = [c for c in CASES if isinstance(c[8], int) and c[8] <= ac.S and c[2] <= 600]
    if mutant == MUTANTS[4]:
        return [c for c in CASES if c[9][5]]
    return small


@pytest.mark.parametrize("mutant", MUTANTS)
def test_each_wrong_kernel_fails_the_bound_on_a_named_row(mutant):
    failing, tried = [], 0
    for c in _mutant_rows(mutant):
        worst, _ = _run(c, mutant)
        if worst is None:
            continue
        tried += 1
        if worst > 1.0:
            failing.append((case_id(c), worst))
    print(f"\nmutant '{mutant}': fails on {len(failing)} of the {tried} rows it applies to; first: {failing[:3]}")
    assert tried > 0
    assert failing, f"'{mutant}' passes the bound on every row it applies to"
    assert len(failing) == tried, f"'{mutant}' passes on some row it applies to"


# --- (d), (e) ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_geometry_query_reports_the_table(c):
    n, cuts, nouts = ac.plan(c, 256)
    assert nouts[-1] == max(nouts) and nouts[-1] % 16
    g = geometry(c, nouts[-1], 256)
    assert reported(g) == c[9], dict(zip(("tile", "span", "nchg", "groups", "tiles", "gy", "taps_in_lds", "lds_bytes"), g))
    tile, span, nchg, groups, tiles, gy, tlds, lds = g
    assert groups == -(-c[5] // nchg) and tiles == -(-nouts[-1] // tile)
    if c[8] == ac.LOOP1:
        assert gy == 1 and groups == 3
    if c[8] == ac.LOOP2:
        assert gy == 2 and groups == 3


def test_geometry_query_figures_of_the_issue_and_argument_checks():
    from dsp_jl_amd import _lib
    import dsp_jl_amd as d
    byid = {case_id(c): c for c in CASES}
    g = geometry(byid["r1.37_p32_h192_f64_c64_c4_default_fresh_n2437"], 2437, 256)
    assert g == (1024, 760, 2, 2, 3, 2, 1, 40448)
    g = geometry(byid["r1.0_p32_h4096_f32_f32_c1_default_fresh_n2437"], 2437, 256)
    assert g == (1024, 1156, 1, 1, 3, 1, 1, 50448)
    assert geometry(byid["r0.004_p16_h48_f64_f64_c1_tile16_fresh_n200"], 200, 256)[1] == 4008
    out = (C.c_int64 * 8)()
    lib = _lib.lib()
    for bad in ((0, 32, 1.0, _lib.F32, _lib.F32, 1, 10), (4, 0, 1.0, _lib.F32, _lib.F32, 1, 10), (4, 32, 0.0, _lib.F32, _lib.F32, 1, 10),
                (4, 32, 1.0, _lib.F32, _lib.F32, 0, 10), (4, 32, 1.0, _lib.F32, _lib.F32, 1, -1)):
        with pytest.raises(d.ArgumentError):
            _lib.check(lib.mdsp_arb_kernel_geometry(*bad, 256, out))
    with pytest.raises(d.ArgumentError):
        _lib.check(lib.mdsp_arb_kernel_geometry(4, 32, 1.0, _lib.F32, _lib.F32, 1, 10, 256, None))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_span_covers_every_tile(c):
    """The kernel stages `span` samples per tile before it knows the tile's extent, and falls back to reading memory (silently: same results, slower)
    when the last output's window ends beyond them.  With span_of right that never happens: for every chunk and tile, x_idx(last) - x_idx(first) + tp
    <= span."""
    rate, nphi, hlen = c[:3]
    tp = -(-hlen // nphi)
    n, cuts, nouts = ac.plan(c)
    acc, dfc, _ = ac.initial_state(c)
    for (a, b), no in zip(zip(cuts[:-1], cuts[1:]), nouts):
        xs, _, acc, dfc = trajectory(acc, dfc, rate, nphi, b - a)
        if no == 0:
            continue
        tile, span = geometry(c, no, 256)[:2]
        if span == 0:
            continue
        first = xs[::tile]
        last = xs[np.minimum(np.arange(tile - 1, no + tile - 1, tile), no - 1)]
        assert int(np.max(last - first)) + tp <= span, (a, b, int(np.max(last - first)) + tp, span)
