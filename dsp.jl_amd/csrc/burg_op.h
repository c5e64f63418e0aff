// Burg's method (src/lpc.jl:53-92) as p passes over two work arrays: the arithmetic, the geometry, the order of every addition and the host emulation.
//
// INDEX FORM.  The reference shortens ef from the back and eb from the front; here neither array moves.  At order m (1-based) element i of ef pairs
// with element i + m of eb, i = 0 .. N-m-1 ("pair i"):
//     cf = ef[N-m]        cb = eb[m-1]        dot_m = sum over i of conj(eb[i+m]) ef[i]          (:70-74)
// and the update (:81-85) touches exactly the pairs of order m.  Every update is element-wise, so the two forms give the same bits.
//
// LAUNCHES.  sweep 0 (reads x: the partials of dot(x, x) and of dot_1), then for m = 1 .. p: finish m (folds the partials of dot_m, adds the products
// at the segment boundaries, takes the scalar step :72-78, :87-88) and, for m < p, sweep m (updates the pairs of order m with k_m and leaves the partials
// of dot_(m+1)).  Sweep 1 reads both operands from x and writes the work arrays; x is never written.  p = 0: sweep 0 and a finish that only folds.
//
// ARITHMETIC, in the element type F (Float32, Float64, ComplexF32, ComplexF64; R its real type); every operation a function of its own:
//     real     ef' = fma(k, eb, ef)             eb' = fma(k, ef, eb)                                         (ef, eb: the values before the update)
//     complex  cfma(z, w, x) = (fma(z.re, w.re, -fma(z.im, w.im, -x.re)),  fma(z.re, w.im, fma(z.im, w.re, x.im)))      Julia's muladd(z, w, x)
//              ef' = cfma(k, eb, ef)            eb' = cfma(conj(k), ef, eb)
//     term i of dot_(m+1), in Float64 (the operands converted exactly):   conj(eb'[i+m+1]) ef'[i]
//              acc.re = fma(b.re, e.re, fma(b.im, e.im, acc.re))          acc.im = fma(b.re, e.im, fma(-b.im, e.re, acc.im))          (real: the first fma only)
//     sweep 0 also adds |x_i|^2:   acc.xx = fma(x.re, x.re, fma(x.im, x.im, acc.xx))
// The folded sums are rounded once to F (dot(x, x): to R) and the scalar step runs in F / R in the reference's order:
//     den = fma(ratio, den, -(abs2(cf) + abs2(cb)))      k = ((-2) dot) / den      a[j] = cfma(k, conj(a_old[m-j]), a_old[j]), j = 1 .. m
//     ratio = 1 - abs2(k)      prediction_err = prediction_err ratio               abs2(z) = z.re z.re + z.im z.im, two products and a sum
//
// GEOMETRY.  The pair range of order 1, [0, N-1), is cut into S segments of seglen pairs, once for all orders: segment s of order m covers
// [s seglen, min((s+1) seglen, N-m)) -- the trailing segments shrink and empty as m grows -- and the last segment of sweep 0 also takes element N-1.
// A segment is walked by one wavefront in tiles of 64 V pairs, V = 16 bytes / sizeof(F): lane l of tile t owns the V pairs from
// s seglen + (64 t + l) V on.  Ownership is by INDEX, never by address, so a result does not depend on where x lies.
//
// ORDER OF ADDITIONS.  A lane adds, tile after tile, into its own accumulator (from zero): first (lane 0, from the second tile on) the term of the
// tile before's last pair, whose ef' lane 63 carried over; then the terms of its pairs but the last in ascending i; then the term of its last pair
// with the eb' of the next lane's first pair (a lane exchange), if that pair is in the segment.  At the segment's end the 64 accumulators are folded as
// fold64 of reduce_op.h, and the partial is STORED.  The term of a segment's last pair needs the eb' of the NEXT segment's first pair: no sweep computes
// it.  The finish: lane l adds the partials l, l + 64, .. (finish_walk), then the boundary terms l, l + 64, .. from the finished arrays, then fold64.
// No atomics, no flags, nothing waits for another workgroup; a record depends on (x, p, the cut) only.
//
// Everything here is shared by the kernels (lpc.hip) and the host emulation (mdsp_burg_emulate_host), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "reduce_op.h"

#if defined(__HIPCC__)
#define BURG_HD __host__ __device__ inline
#else
#define BURG_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define BURG_UNROLL _Pragma("unroll")
#else
#define BURG_UNROLL
#endif

namespace mdsp {
namespace burg {

using reduceop::add_rn;
using reduceop::c32;
using reduceop::c64;
using reduceop::mul_rn;

BURG_HD double fma_rn(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);
#else
    return __builtin_fma(a, b, c);
#endif
}
BURG_HD float fma_rn(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return __builtin_fmaf(a, b, c);
#endif
}
BURG_HD double div_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
BURG_HD float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

template <typename F> struct Elem;
template <> struct Elem<float> { using R = float; static constexpr bool CPLX = false; };
template <> struct Elem<double> { using R = double; static constexpr bool CPLX = false; };
template <> struct Elem<c32> { using R = float; static constexpr bool CPLX = true; };
template <> struct Elem<c64> { using R = double; static constexpr bool CPLX = true; };

BURG_HD float conj_of(float z) { return z; }
BURG_HD double conj_of(double z) { return z; }
template <typename R> BURG_HD reduceop::cpx<R> conj_of(reduceop::cpx<R> z) { return reduceop::cpx<R>{z.re, -z.im}; }

// z w + x
BURG_HD float cfma(float z, float w, float x) { return fma_rn(z, w, x); }
BURG_HD double cfma(double z, double w, double x) { return fma_rn(z, w, x); }
template <typename R> BURG_HD reduceop::cpx<R> cfma(reduceop::cpx<R> z, reduceop::cpx<R> w, reduceop::cpx<R> x) {
    return reduceop::cpx<R>{fma_rn(z.re, w.re, -fma_rn(z.im, w.im, -x.re)), fma_rn(z.re, w.im, fma_rn(z.im, w.re, x.im))};
}

BURG_HD float abs2_of(float z) { return mul_rn(z, z); }
BURG_HD double abs2_of(double z) { return mul_rn(z, z); }
template <typename R> BURG_HD R abs2_of(reduceop::cpx<R> z) { return add_rn(mul_rn(z.re, z.re), mul_rn(z.im, z.im)); }

BURG_HD float make_elem(float re, float, float*) { return re; }
BURG_HD double make_elem(double re, double, double*) { return re; }
template <typename R> BURG_HD reduceop::cpx<R> make_elem(R re, R im, reduceop::cpx<R>*) { return reduceop::cpx<R>{re, im}; }
template <typename F> BURG_HD F elem(typename Elem<F>::R re, typename Elem<F>::R im) { return make_elem(re, im, static_cast<F*>(nullptr)); }

BURG_HD double re_of(float z) { return (double)z; }
BURG_HD double re_of(double z) { return z; }
BURG_HD double im_of(float) { return 0.0; }
BURG_HD double im_of(double) { return 0.0; }
template <typename R> BURG_HD double re_of(reduceop::cpx<R> z) { return (double)z.re; }
template <typename R> BURG_HD double im_of(reduceop::cpx<R> z) { return (double)z.im; }

// the partial sums: {Re dot, Im dot, dot(x, x)} as an operator for finish_walk / fold64 of reduce_op.h
struct Sums { double s[3]; };
struct OpSums {
    using Acc = Sums;
    BURG_HD static Acc identity() { return Acc{{0.0, 0.0, 0.0}}; }
    BURG_HD static Acc combine(Acc a, Acc b, const reduceop::Params&) {
        for (int i = 0; i < 3; ++i) a.s[i] = add_rn(a.s[i], b.s[i]);
        return a;
    }
};

// acc += conj(b) e
template <typename F> BURG_HD void add_term(F b, F e, Sums& acc) {
    if constexpr (Elem<F>::CPLX) {
        acc.s[0] = fma_rn(re_of(b), re_of(e), fma_rn(im_of(b), im_of(e), acc.s[0]));
        acc.s[1] = fma_rn(re_of(b), im_of(e), fma_rn(-im_of(b), re_of(e), acc.s[1]));
    } else {
        acc.s[0] = fma_rn(re_of(b), re_of(e), acc.s[0]);
    }
}
template <typename F> BURG_HD void add_abs2(F x, Sums& acc) {
    if constexpr (Elem<F>::CPLX) acc.s[2] = fma_rn(re_of(x), re_of(x), fma_rn(im_of(x), im_of(x), acc.s[2]));
    else acc.s[2] = fma_rn(re_of(x), re_of(x), acc.s[2]);
}

template <typename F> struct Lane {
    static constexpr int V = 16 / (int)sizeof(F);
    static constexpr int TILE = 64 * V;
};

// the update of a lane's cnt pairs in registers (:81-85)
template <typename F> BURG_HD void lane_update(F k, F* e, F* b, int cnt) {
    constexpr int V = Lane<F>::V;
    const F kc = conj_of(k);
    BURG_UNROLL
    for (int t = 0; t < V; ++t) {
        if (t < cnt) {
            const F eo = e[t], bo = b[t];
            e[t] = cfma(k, bo, eo);
            b[t] = cfma(kc, eo, bo);
        }
    }
}

// the terms of a lane in the order stated above.  carried: lane 0 adds the term of the tile before's last pair (its ef' in carry_e) first.
// has_next: the pair behind the lane's last one is in the segment, its eb' in next_b.
template <typename F> BURG_HD void lane_terms(const F* e, const F* b, int cnt, bool first_sweep, bool carried, F carry_e, bool has_next, F next_b, Sums& acc) {
    constexpr int V = Lane<F>::V;
    if (carried && cnt > 0) add_term(b[0], carry_e, acc);
    BURG_UNROLL
    for (int t = 0; t < V; ++t) {
        if (t < cnt) {
            if (first_sweep) add_abs2(e[t], acc);
            if (t + 1 < cnt) add_term(b[t + 1 < V ? t + 1 : t], e[t], acc);
            else if (has_next) add_term(next_b, e[t], acc);   // t == cnt - 1: the lane's last pair
        }
    }
}

// ---- the scalar step.  State: what one finish hands to the next (device memory of the plan)
template <typename R> struct State { R den, ratio, err, pad; };

template <typename F> BURG_HD void state_init(double xx, int64_t n, State<typename Elem<F>::R>& st) {
    using R = typename Elem<F>::R;
    const R unnormed = (R)xx;                      // abs(dot(x, x)) :55
    st.err = div_rn(unnormed, (R)n);               // :56
    st.den = mul_rn((R)2, unnormed);               // :66
    st.ratio = (R)1;                               // :67
    st.pad = (R)0;
}

// :72-74, :87-88; returns k
template <typename F> BURG_HD F scalar_step(double dre, double dim, F cf, F cb, State<typename Elem<F>::R>& st) {
    using R = typename Elem<F>::R;
    st.den = fma_rn(st.ratio, st.den, -add_rn(abs2_of(cf), abs2_of(cb)));
    const F k = elem<F>(div_rn(mul_rn((R)-2, (R)dre), st.den), div_rn(mul_rn((R)-2, (R)dim), st.den));
    st.ratio = add_rn((R)1, -abs2_of(k));
    st.err = mul_rn(st.err, st.ratio);
    return k;
}

// :77-78 for the pair (j, m - j) of a, 0 <= j <= m / 2; first: a is [1, 0, ..] and is not read; last: the conj! of :91 goes with the store
template <typename F> BURG_HD void a_update_pair(F* a, int64_t m, int64_t j, F k, bool first, bool last) {
    using R = typename Elem<F>::R;
    const int64_t lo = j, hi = m - j;
    const F olo = first ? elem<F>(lo == 0 ? (R)1 : (R)0, (R)0) : a[lo];
    const F ohi = (first || hi == m) ? elem<F>((R)0, (R)0) : a[hi];
    if (lo >= 1) {
        const F v = cfma(k, conj_of(ohi), olo);
        a[lo] = last ? conj_of(v) : v;
    } else if (first || last) a[0] = last ? conj_of(olo) : olo;
    if (hi != lo) {
        const F v = cfma(k, conj_of(olo), ohi);
        a[hi] = last ? conj_of(v) : v;
    }
}

// ---- geometry: pure host arithmetic, the same on every machine (256 compute units are assumed); the rule of sos_scan.h / quinn_scan.h for one line
struct Geom {
    int64_t n = 0, S = 1, seglen = 1, tile = 0, workspace = 0;
};
constexpr int64_t UNITS_TARGET = 256 * 16;   // segment wavefronts of an automatic cut
constexpr int64_t MINSEG_TILES = 16;         // shortest segment of an automatic cut, in tiles (a forced cut goes down to 1 pair)

inline Geom make_geometry(int64_t elem_bytes, int64_t n, int64_t segments) {
    Geom g;
    g.n = n;
    g.tile = 64 * (16 / elem_bytes);
    const int64_t pairs = n > 1 ? n - 1 : 1;
    int64_t want = 1;
    if (segments > 0) want = segments < pairs ? segments : pairs;
    else {
        want = UNITS_TARGET;
        const int64_t cap = pairs / (MINSEG_TILES * g.tile);
        want = want < cap ? want : cap;
        if (want < 1) want = 1;
    }
    g.seglen = (pairs + want - 1) / want;
    if (segments <= 0 && want > 1) g.seglen = (g.seglen + g.tile - 1) / g.tile * g.tile;   // an automatic cut falls on tile boundaries
    g.S = (pairs + g.seglen - 1) / g.seglen;
    // ef and eb (each rounded up to 256 bytes), a partial per segment, the state
    const int64_t arr = (n * elem_bytes + 255) / 256 * 256;
    g.workspace = 2 * arr + g.S * (int64_t)sizeof(Sums) + 64;
    return g;
}

// [j0, j1) of segment s in the sweep of order m (m = 0: the pass over x)
BURG_HD void segment_range(int64_t n, int64_t S, int64_t seglen, int64_t s, int64_t m, int64_t* j0, int64_t* j1) {
    const int64_t npairs = n - m;
    *j0 = s * seglen;
    int64_t e = *j0 + seglen;
    if (e > npairs || (m == 0 && s == S - 1)) e = npairs;
    *j1 = e;
}

// elements of the record: a (p + 1), the reflection coefficients (p), prediction_err in the real part of the last
inline int64_t record_elems(int64_t p) { return 2 * p + 2; }

// ---- host emulation
// sweep m on host arrays: ein / bin are read, eout / bout written (m = 0: nothing is written; m = 1: ein = bin = x), part: S partials
template <typename F> inline void sweep_host(const Geom& g, int64_t m, F k, const F* ein, const F* bin, F* eout, F* bout, Sums* part) {
    constexpr int V = Lane<F>::V;
    constexpr int TILE = Lane<F>::TILE;
    const reduceop::Params prm{0.0, 0};
    for (int64_t s = 0; s < g.S; ++s) {
        int64_t j0, j1;
        segment_range(g.n, g.S, g.seglen, s, m, &j0, &j1);
        Sums lanes[64];
        for (int l = 0; l < 64; ++l) lanes[l] = OpSums::identity();
        F carry_e{};
        for (int64_t t0 = j0; t0 < j1; t0 += TILE) {
            F e[64][V], b[64][V];
            int cnt[64];
            for (int l = 0; l < 64; ++l) {
                const int64_t i = t0 + (int64_t)l * V;
                const int64_t c = j1 - i;
                cnt[l] = (int)(c < 0 ? 0 : c > V ? V : c);
                for (int t = 0; t < cnt[l]; ++t) {
                    e[l][t] = ein[i + t];
                    b[l][t] = bin[i + t + m];
                }
                if (m >= 1) {
                    lane_update<F>(k, e[l], b[l], cnt[l]);
                    for (int t = 0; t < cnt[l]; ++t) {
                        eout[i + t] = e[l][t];
                        bout[i + t + m] = b[l][t];
                    }
                }
            }
            for (int l = 0; l < 64; ++l) {
                const bool has_next = l < 63 && cnt[l + 1] > 0;
                lane_terms<F>(e[l], b[l], cnt[l], m == 0, l == 0 && t0 > j0, carry_e, has_next, has_next ? b[l + 1][0] : F{}, lanes[l]);
            }
            if (cnt[63] == V) carry_e = e[63][V - 1];
        }
        part[s] = reduceop::fold64<OpSums>(lanes, prm);
    }
}

// the folded sums of the finish of order m (m >= 1; m = 0 or 1 reads x through ef = eb = x): the partials, then the boundary terms
template <typename F> inline Sums finish_sums_host(const Geom& g, int64_t m, const Sums* part, const F* ef, const F* eb) {
    const reduceop::Params prm{0.0, 0};
    Sums lanes[64];
    for (int l = 0; l < 64; ++l) {
        lanes[l] = reduceop::finish_walk<OpSums>(part, g.S, l, prm);
        if (m >= 1)
            for (int64_t s = l; s + 1 < g.S; s += 64) {
                const int64_t ib = (s + 1) * g.seglen;
                if (ib < g.n - m + 1) add_term(eb[ib + m - 1], ef[ib - 1], lanes[l]);
            }
    }
    return reduceop::fold64<OpSums>(lanes, prm);
}

// the whole recursion; rec: record_elems(p) elements of F
template <typename F> inline void emulate(const Geom& g, const F* x, int64_t p, F* rec) {
    using R = typename Elem<F>::R;
    std::vector<F> ef((size_t)g.n), eb((size_t)g.n);
    std::vector<Sums> part((size_t)g.S);
    State<R> st;
    sweep_host<F>(g, 0, F{}, x, x, nullptr, nullptr, part.data());
    F* a = rec;
    F* refl = rec + p + 1;
    if (p == 0) {
        const Sums sm = finish_sums_host<F>(g, 0, part.data(), x, x);
        state_init<F>(sm.s[2], g.n, st);
        a[0] = elem<F>((R)1, (R)0);
    }
    for (int64_t m = 1; m <= p; ++m) {
        const F* e = m == 1 ? x : ef.data();
        const F* b = m == 1 ? x : eb.data();
        const Sums sm = finish_sums_host<F>(g, m, part.data(), e, b);
        if (m == 1) state_init<F>(sm.s[2], g.n, st);
        const F k = scalar_step<F>(sm.s[0], sm.s[1], e[g.n - m], b[m - 1], st);
        refl[m - 1] = k;
        for (int64_t j = 0; j <= m / 2; ++j) a_update_pair<F>(a, m, j, k, m == 1, m == p);
        if (m < p) sweep_host<F>(g, m, k, e, b, ef.data(), eb.data(), part.data());
    }
    rec[2 * p + 1] = elem<F>(st.err, (R)0);
}

}  // namespace burg
}  // namespace mdsp
