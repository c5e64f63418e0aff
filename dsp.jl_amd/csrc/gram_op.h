// The Gram matrix R = X X^H of the Hankel matrix X[i, k] = x[i + k] (M rows, L = n - M + 1 columns) that esprit (src/estimation.jl:69-71) takes its
// signal subspace from: the arithmetic, the geometry, the order of every addition and the host emulation.
//
// DECOMPOSITION.  With p_d[k] = x[k + d] conj(x[k]), entry (j + d, j) of R, 0 <= d <= M - 1, 0 <= j <= M - 1 - d, is the window sum of p_d over
// k = j .. j + L - 1.  2 M - 1 <= n gives L >= M, so every window holds the BODY k = M - 1 .. L - 1; what differs is a HEAD and a TAIL of at most M - 1
// products each:
//     B_d    = sum of p_d[k], k = M - 1 .. L - 1                         one pass over the signal for all M lags
//     H_d[j] = sum of p_d[k], k = j .. M - 2                             a running sum, k walked DOWN from M - 2
//     T_d[j] = sum of p_d[k], k = L .. j + L - 1                         a running sum, k walked UP from L
//     R[j + d, j] = (H_d[j] + B_d) + T_d[j]            R[j, j + d] = conj of it            the diagonal's imaginary part is stored as +0.0
// No window sum is the difference of two running totals: every entry is a sum of its own products only.
//
// ARITHMETIC.  Float64 throughout (Float32 operands convert exactly and their products are exact in Float64); every operation a function of its own:
//     acc += a conj(c)   is   acc.re = fma(a.re, c.re, fma(a.im, c.im, acc.re))      acc.im = fma(a.im, c.re, fma(-a.re, c.im, acc.im))
// (real types: the first fma only), with a = x[k + d], c = x[k]; sums of sums are add_rn per component.  An empty sum is +0.0 and is still added.
//
// GEOMETRY.  The body range [M - 1, L) is cut into S segments of seglen; a workgroup of 4 wavefronts per (segment, block of LAG_BLOCK lags) walks its
// segment in tiles of TILE = 64 E samples.  In a tile lane l owns the samples t0 + 64 e + l, e = 0 .. E - 1 -- by INDEX, never by address -- and a
// wavefront owns the lag groups (of G lags) g, g + 4, .. of the block.
//
// ORDER OF ADDITIONS of B_d.  Per tile a lane adds the terms of its samples in ascending e into an accumulator that starts at +0.0; the 64 accumulators
// are folded (off = 32, 16, .., 1: acc[l] += acc[l + off], l < off); the tile's sum is added to the segment's running sum (from +0.0), tile after tile;
// the segment's sum is STORED: one partial per (segment, lag).  The assembly adds the partials in segment order: B = part[0]; B += part[s], s = 1 ...
// No atomics, no flags, nothing waits on another workgroup: R depends on (x, M, the cut) only.
//
// Everything here is shared by the kernels (gram.hip) and the host emulation (mdsp_hankel_gram_emulate_host), which runs the same text.
#pragma once

#include <cstdint>
#include <vector>

#include "burg_op.h"

namespace mdsp {
namespace gram {

using burg::Elem;
using burg::fma_rn;
using burg::im_of;
using burg::re_of;
using reduceop::add_rn;
using reduceop::c32;
using reduceop::c64;

constexpr int WAVES = 4;                  // wavefronts of a body workgroup
constexpr int E = 8;                      // samples of a tile a lane owns
constexpr int TILE = 64 * E;              // samples of a tile
constexpr int G = 8;                      // lags a lane accumulates at a time
constexpr int LAG_BLOCK = 1024;           // lags of one workgroup: the halo staged beside a tile is at most LAG_BLOCK - 1 samples

struct Acc { double re, im; };

template <bool CPLX> BURG_HD void add_term(double are, double aim, double cre, double cim, Acc& acc) {
    if constexpr (CPLX) {
        acc.re = fma_rn(are, cre, fma_rn(aim, cim, acc.re));
        acc.im = fma_rn(aim, cre, fma_rn(-are, cim, acc.im));
    } else {
        acc.re = fma_rn(are, cre, acc.re);
    }
}
template <typename F> BURG_HD void add_product(F a, F c, Acc& acc) { add_term<Elem<F>::CPLX>(re_of(a), im_of(a), re_of(c), im_of(c), acc); }

template <bool CPLX> BURG_HD Acc add_acc(Acc a, Acc b) {
    a.re = add_rn(a.re, b.re);
    if constexpr (CPLX) a.im = add_rn(a.im, b.im);
    return a;
}

// ---- geometry: pure host arithmetic, the same on every machine (256 compute units are assumed, as in burg_op.h)
struct Geom {
    int64_t n = 0, M = 1, L = 0, S = 1, seglen = 1, workspace = 0;
    bool cplx = false;
};
constexpr int64_t UNITS_TARGET = 256 * 4;   // segments of an automatic cut
constexpr int64_t MINSEG_TILES = 2;         // shortest segment of an automatic cut, in tiles (a forced cut goes down to 1 sample)

// requires 1 <= M and 2 M - 1 <= n
inline Geom make_geometry(bool cplx, int64_t n, int64_t M, int64_t segments) {
    Geom g;
    g.n = n;
    g.M = M;
    g.L = n - M + 1;
    g.cplx = cplx;
    const int64_t body = g.L - M + 1;       // >= 1
    int64_t want = 1;
    if (segments > 0) want = segments < body ? segments : body;
    else {
        want = UNITS_TARGET;
        const int64_t cap = body / (MINSEG_TILES * TILE);
        want = want < cap ? want : cap;
        if (want < 1) want = 1;
    }
    g.seglen = (body + want - 1) / want;
    if (segments <= 0 && want > 1) g.seglen = (g.seglen + TILE - 1) / TILE * TILE;   // an automatic cut falls on tile boundaries
    g.S = (body + g.seglen - 1) / g.seglen;
    g.workspace = g.S * M * (cplx ? 16 : 8);   // a partial per (segment, lag)
    return g;
}

// [k0, k1) of segment s
BURG_HD void segment_range(int64_t M, int64_t L, int64_t seglen, int64_t s, int64_t* k0, int64_t* k1) {
    *k0 = M - 1 + s * seglen;
    const int64_t e = *k0 + seglen;
    *k1 = e < L ? e : L;
}

// ---- the edges and the assembly of diagonal d: one lane.  part: S x M partials of NC = 1 (real) or 2 doubles; r: column-major, ldr >= M, elements of
// NC doubles.  The lane writes R[j + d, j] and R[j, j + d] for j = 0 .. M - 1 - d and nothing else; between its two walks it keeps (H + B) in R[j + d, j].
// x, part and r never overlap (__restrict__: the loads of x need not wait for the stores into r).
template <typename F>
BURG_HD void assemble_diagonal(const F* __restrict__ x, int64_t M, int64_t L, int64_t S, const double* __restrict__ part, int64_t d, double* __restrict__ r,
                               int64_t ldr) {
    constexpr bool CP = Elem<F>::CPLX;
    constexpr int NC = CP ? 2 : 1;
    Acc B{part[d * NC], CP ? part[d * NC + 1] : 0.0};
    for (int64_t s = 1; s < S; ++s) B = add_acc<CP>(B, Acc{part[(s * M + d) * NC], CP ? part[(s * M + d) * NC + 1] : 0.0});
    Acc H{0.0, 0.0};
    for (int64_t j = M - 1; j >= 0; --j) {                      // heads, k = j walked down
        if (j <= M - 2) add_product<F>(x[j + d], x[j], H);
        if (j <= M - 1 - d) {
            const Acc v = add_acc<CP>(H, B);
            double* q = r + ((j + d) + j * ldr) * NC;
            q[0] = v.re;
            if constexpr (CP) q[1] = v.im;
        }
    }
    Acc T{0.0, 0.0};
    for (int64_t j = 0; j <= M - 1 - d; ++j) {                  // tails, k = j + L - 1 walked up
        if (j >= 1) add_product<F>(x[j + L - 1 + d], x[j + L - 1], T);
        double* q = r + ((j + d) + j * ldr) * NC;
        Acc v{q[0], CP ? q[1] : 0.0};
        v = add_acc<CP>(v, T);
        if (d == 0) v.im = 0.0;
        q[0] = v.re;
        if constexpr (CP) q[1] = v.im;
        if (d > 0) {
            double* m = r + (j + (j + d) * ldr) * NC;
            m[0] = v.re;
            if constexpr (CP) m[1] = -v.im;
        }
    }
}

// ---- host emulation
inline Acc fold64(Acc* a, bool cplx) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) a[l] = cplx ? add_acc<true>(a[l], a[l + off]) : add_acc<false>(a[l], a[l + off]);
    return a[0];
}

template <typename F> inline void body_host(const Geom& g, const F* x, double* part) {
    constexpr bool CP = Elem<F>::CPLX;
    constexpr int NC = CP ? 2 : 1;
    for (int64_t s = 0; s < g.S; ++s) {
        int64_t k0, k1;
        segment_range(g.M, g.L, g.seglen, s, &k0, &k1);
        for (int64_t d = 0; d < g.M; ++d) {
            Acc run{0.0, 0.0};
            for (int64_t t0 = k0; t0 < k1; t0 += TILE) {
                const int64_t cnt = k1 - t0 < TILE ? k1 - t0 : TILE;
                Acc lanes[64];
                for (int l = 0; l < 64; ++l) {
                    lanes[l] = Acc{0.0, 0.0};
                    for (int e = 0; e < E; ++e) {
                        const int64_t i = 64 * e + l;
                        if (i < cnt) add_product<F>(x[t0 + i + d], x[t0 + i], lanes[l]);
                    }
                }
                run = add_acc<CP>(run, fold64(lanes, CP));
            }
            part[(s * g.M + d) * NC] = run.re;
            if constexpr (CP) part[(s * g.M + d) * NC + 1] = run.im;
        }
    }
}

template <typename F> inline void emulate(const Geom& g, const F* x, double* r, int64_t ldr) {
    std::vector<double> part((size_t)(g.workspace / 8));
    body_host<F>(g, x, part.data());
    for (int64_t d = 0; d < g.M; ++d) assemble_diagonal<F>(x, g.M, g.L, g.S, part.data(), d, r, ldr);
}

}  // namespace gram
}  // namespace mdsp
