"""CPU checks of tests/polyphase_ref.py, the extended-precision reference of the polyphase GPU sweep (tests/test_gpu_polyphase_paths.py):

  * it agrees with the Float64 oracle (oracle.stream_filt.FIRFilter.filt) on random short shapes -- interpolator, decimator and rational
    kinds, setphase, streams cut into 1-sample and ragged chunks, real and complex signals, Float32 and Float64 taps -- with identical states
    after every chunk;
  * the element-wise bound the sweep applies, |y - ref| <= 2 (tp + 1) u absdot + 4 u_min, passes a correct Float32 computation and fails
    three subtly wrong ones (a dropped tap, a wrong phase on one output, one channel shifted by a sample): the bound is not vacuous.
"""
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

from oracle import stream_filt as osf
from polyphase_ref import accumulation_unit, excess, polyphase_ref


def _shape(rng):
    kind = rng.integers(0, 3)
    if kind == 0:
        L, M = int(rng.integers(2, 20)), 1
    elif kind == 1:
        L, M = 1, int(rng.integers(2, 12))
    else:
        while True:
            L, M = int(rng.integers(2, 30)), int(rng.integers(2, 30))
            if gcd(L, M) == 1:
                break
    hlen = int(rng.integers(1, 6 * L + 40))
    return L, M, hlen


def _wide(x):
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_the_oracle(seed):
    rng = np.random.default_rng(9100 + seed)
    L, M, hlen = _shape(rng)
    hdt = np.float32 if seed % 2 else np.float64
    xdt = [np.float32, np.float64, np.complex64, np.complex128][seed % 4]
    h = rng.standard_normal(hlen).astype(hdt)
    n = int(rng.integers(1, 400))
    x = rng.standard_normal(n)
    if np.dtype(xdt).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    x = x.astype(xdt)
    of = osf.FIRFilter(h.astype(np.float64), Fraction(L, M))
    if seed % 3 == 0:
        of.setphase(float(rng.uniform(0, 4)))
    # chunks: 1-sample runs, an empty chunk and ragged pieces
    if seed % 5 == 0:
        cuts = list(range(n + 1))
    else:
        cuts = sorted({0, n, 1, *[int(c) for c in rng.integers(0, n + 1, size=4)]} & set(range(n + 1)))
        cuts = [0] + cuts
    phi, dfc = of.phi_idx, of.input_deficit
    hist = None
    tp = -(-hlen // L)
    u = 2.0 ** -53
    for a, b in zip(cuts[:-1], cuts[1:]):
        yo = of.filt(_wide(x[a:b]))
        y, ad, (phi, dfc, hist) = polyphase_ref(h, L, M, x[a:b], phi, dfc, hist)
        assert (phi, dfc) == (of.phi_idx, of.input_deficit), (a, b)
        assert np.array_equal(_wide(hist), of.history), (a, b)
        assert y.shape == yo.shape
        if y.size:
            # the oracle's Float64 dot products against the long-double ones: within (tp + 1) 2^-53 absdot element-wise, ~1e-15 relative
            worst, _ = excess(yo, y, ad, tp, u / 2, 0.0)
            assert worst <= 1.0, (L, M, hlen, a, b, worst)
            ref = np.asarray(y, dtype=np.complex128 if np.iscomplexobj(y) else np.float64)
            assert np.linalg.norm(yo - ref) <= 2e-15 * np.sqrt(tp) * max(np.linalg.norm(ref), 1e-300)


def test_reference_state_of_short_chunks_matches_the_closed_form():
    # a chunk shorter than the deficit produces nothing and only lowers the deficit (stream_filt.jl:483-487)
    h = np.arange(1.0, 50.0)
    y, ad, (phi, dfc, hist) = polyphase_ref(h, 3, 7, np.ones(2), phi_idx=2, input_deficit=5)
    assert y.size == 0 and (phi, dfc) == (2, 3) and np.array_equal(hist, [0.0] * 14 + [1.0, 1.0])
    assert polyphase_ref(h, 3, 7, np.ones(0), 2, 5)[2][:2] == (2, 5)


# --- self-check of the comparator -----------------------------------------------------------------------------------------------------------

def _f32_kernel(h, L, M, x, drop_phase=None, wrong_output=None, shift_channel=None):
    """A Float32 'kernel': per output an oldest-sample-first fmaf-free chain of Float32 products and sums, from zero state, on (nch, n) samples.
    The three knobs make it subtly wrong: drop the last tap of one phase, use the next phase on one output, delay one channel by a sample."""
    pfb = osf.taps2pfb(h.astype(np.float32), L)
    tp = pfb.shape[0]
    nch, n = x.shape
    z = np.concatenate([np.zeros((nch, tp - 1), dtype=x.dtype), x], axis=1)
    nout = -(-(n * L) // M)
    phi, idx = osf.polyphase_closed_form(1, 1, L, M, np.arange(nout))
    col = phi - 1
    if wrong_output is not None:
        col = col.copy()
        col[wrong_output] = (col[wrong_output] + 1) % L
    acc = np.zeros((nch, nout), dtype=x.dtype)
    for k in range(tp):
        hk = pfb[k, col].copy()
        if drop_phase is not None and k == tp - 1:
            hk[col == drop_phase] = 0
        acc = (acc + (hk * z[:, idx - 1 + k]).astype(x.dtype)).astype(x.dtype)
    if shift_channel is not None:
        acc[shift_channel] = np.concatenate([np.zeros(1, dtype=x.dtype), acc[shift_channel, :-1]])
    return acc


@pytest.mark.parametrize("L,M,hlen,cplx", [(5, 3, 61, False), (1, 4, 37, True), (7, 1, 50, False), (160, 147, 5120, True)])
def test_the_bound_passes_float32_and_fails_three_wrong_kernels(L, M, hlen, cplx):
    rng = np.random.default_rng(L * 31 + M)
    h = rng.standard_normal(hlen).astype(np.float32)
    nch, n = 3, 4000
    x = rng.standard_normal((nch, n))
    if cplx:
        x = x + 1j * rng.standard_normal((nch, n))
    x = x.astype(np.complex64 if cplx else np.float32)
    y, ad, _ = polyphase_ref(h, L, M, x)
    tp = -(-hlen // L)
    u, umin = accumulation_unit(np.float32, x.dtype)
    worst, ratio = excess(_f32_kernel(h, L, M, x), y, ad, tp, u, umin)
    assert worst <= 1.0 and ratio > 0                                   # the correct Float32 computation passes
    nout = y.shape[1]
    wrong = {"dropped last tap of one phase": _f32_kernel(h, L, M, x, drop_phase=(L - 1) // 2),
             "next phase on one output": _f32_kernel(h, L, M, x, wrong_output=nout // 2) if L > 1 else None,
             "one channel a sample late": _f32_kernel(h, L, M, x, shift_channel=1)}
    if L == 1:   # (a decimator has one phase: take the off-by-one on the window instead -- one output reads the next input position)
        yw = _f32_kernel(h, L, M, x).copy()
        yw[:, nout // 2] = _f32_kernel(h, L, M, np.concatenate([x[:, 1:], x[:, :1]], axis=1))[:, nout // 2]
        wrong["next phase on one output"] = yw
    for what, yw in wrong.items():
        assert excess(yw, y, ad, tp, u, umin)[0] > 1.0, what
