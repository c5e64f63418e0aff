// Filter responses (Filters/response.jl:27-52, :96-111): a rational function of a point of the unit circle, one evaluation point per lane.
//
// Working type: Cx<R>, R = float or double.  Every operation is a function of its own (the library is compiled with -ffp-contract=on; a function per
// operation keeps host and device to the same roundings), every real operation is rounded once, to nearest:
//
//     horner_step   acc <- acc y + c, c real      re = fma(-acc.im, y.im, fma(acc.re, y.re, c)),    im = fma(acc.im, y.re, acc.re * y.im)
//     horner_step_c acc <- acc q + p, p complex   re = fma(-acc.im, q.im, fma(acc.re, q.re, p.re)), im = fma(acc.im, q.re, fma(acc.re, q.im, p.im))
//     cmul          a b                           re = fma(-a.im, b.im, a.re * b.re),               im = fma(a.im, b.re, a.re * b.im)
//     scale         g a, g real                   (g * a.re, g * a.im)
//     sub_root      x - r                         (x.re - r.re, x.im - r.im)
//     cdiv          n / d   SCALED (Smith 1962): with |d.re| >= |d.im|, r = d.im / d.re, t = fma(d.im, r, d.re),
//                           re = fma(n.im, r, n.re) / t, im = fma(-n.re, r, n.im) / t; otherwise the same with the parts of d exchanged
//                           (r = d.re / d.im, t = fma(d.re, r, d.im), re = fma(n.re, r, n.im) / t, im = fma(n.im, r, -n.re) / t).
//                           Three correctly rounded real divisions; no intermediate |d|^2, so no overflow or underflow a representable quotient does not have.
//     biquad        fma(fma(b0, x, b1), x, b2) / fma(x + a1, x, a2) (response.jl:49-50): t = (fma(b0, x.re, b1), b0 * x.im), num = horner_step(t, x, b2),
//                   u = (x.re + a1, x.im), den = horner_step(u, x, a2), cdiv(num, den)
//
// The three forms:
//     POLY      num(y) / den(y), num = sum b[k] y^k, den = sum a[k] y^k (absent: 1), Horner from the highest coefficient; DERIV: the numerator's
//               coefficient k is mul(R(k), b[k]), rounded once (response.jl:106).
//     SECTIONS  g prod_k biquad_k(x), left to right from one (response.jl:51-52).
//     ZPK       (k prod (x - z_i)) / prod (x - p_i), both products left to right from one (response.jl:47-48).
//
// The cut of POLY: the coefficients are cut into C chunks of L = 2^l; chunk c is P_c(y) = sum_j coef[c L + j] y^j (Horner over its own coefficients,
// zero where the polynomial has none), and the value is Horner over the chunks in q = y^L (l squarings, pow2l below), from the highest chunk:
// acc = P_(C-1); acc <- horner_step_c(acc, q, P_c), c = C-2 .. 0.  C == 1 is the plain Horner chain.
//
// Everything here is shared by the kernels (response.hip) and the host emulation (mdsp_resp_emulate_host), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RESP_HD __host__ __device__ inline
#else
#define RESP_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define RESP_UNROLL8 _Pragma("unroll 8")
#else
#define RESP_UNROLL8
#endif

namespace mdsp {
namespace resp {

enum : int { FORM_POLY = 0, FORM_SECTIONS = 1, FORM_ZPK = 2 };
enum : int { FLAG_DERIV = 1, FLAG_NEG = 2 };
enum : int { OUT_COMPLEX = 0, OUT_ANGLE = 1, OUT_REAL_MINUS = 2 };
enum : int { IN_W = 0, IN_POINTS = 1 };

constexpr int MAXK = 16;             // sections of the largest cascade
constexpr int LANES = 64;            // evaluation points per workgroup: one wavefront
constexpr int64_t MIN_L = 16;        // shortest chunk of a forced cut
constexpr int64_t AUTO_MIN_L = 256;  // shortest chunk of an automatic cut
constexpr int64_t WAVES_TARGET = 256 * 8;   // wavefronts an automatic cut aims at (256 compute units are assumed)

template <typename R> struct Cx { R re, im; };

// ---- one rounding per operation
#if defined(__HIP_DEVICE_COMPILE__)
RESP_HD float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
RESP_HD double fma_rn(double a, double b, double c) { return __fma_rn(a, b, c); }
RESP_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
RESP_HD double mul_rn(double a, double b) { return __dmul_rn(a, b); }
RESP_HD float add_rn(float a, float b) { return __fadd_rn(a, b); }
RESP_HD double add_rn(double a, double b) { return __dadd_rn(a, b); }
RESP_HD float sub_rn(float a, float b) { return __fsub_rn(a, b); }
RESP_HD double sub_rn(double a, double b) { return __dsub_rn(a, b); }
RESP_HD float div_rn(float a, float b) { return __fdiv_rn(a, b); }
RESP_HD double div_rn(double a, double b) { return __ddiv_rn(a, b); }
#else
RESP_HD float fma_rn(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
RESP_HD double fma_rn(double a, double b, double c) { return __builtin_fma(a, b, c); }
RESP_HD float mul_rn(float a, float b) { return a * b; }
RESP_HD double mul_rn(double a, double b) { return a * b; }
RESP_HD float add_rn(float a, float b) { return a + b; }
RESP_HD double add_rn(double a, double b) { return a + b; }
RESP_HD float sub_rn(float a, float b) { return a - b; }
RESP_HD double sub_rn(double a, double b) { return a - b; }
RESP_HD float div_rn(float a, float b) { return a / b; }
RESP_HD double div_rn(double a, double b) { return a / b; }
#endif

template <typename R> RESP_HD Cx<R> horner_step(Cx<R> acc, Cx<R> y, R c) {
    Cx<R> r;
    r.re = fma_rn(-acc.im, y.im, fma_rn(acc.re, y.re, c));
    r.im = fma_rn(acc.im, y.re, mul_rn(acc.re, y.im));
    return r;
}
template <typename R> RESP_HD Cx<R> horner_step_c(Cx<R> acc, Cx<R> q, Cx<R> p) {
    Cx<R> r;
    r.re = fma_rn(-acc.im, q.im, fma_rn(acc.re, q.re, p.re));
    r.im = fma_rn(acc.im, q.re, fma_rn(acc.re, q.im, p.im));
    return r;
}
template <typename R> RESP_HD Cx<R> cmul(Cx<R> a, Cx<R> b) {
    Cx<R> r;
    r.re = fma_rn(-a.im, b.im, mul_rn(a.re, b.re));
    r.im = fma_rn(a.im, b.re, mul_rn(a.re, b.im));
    return r;
}
template <typename R> RESP_HD Cx<R> scale(R g, Cx<R> a) {
    Cx<R> r;
    r.re = mul_rn(g, a.re);
    r.im = mul_rn(g, a.im);
    return r;
}
template <typename R> RESP_HD Cx<R> sub_root(Cx<R> x, Cx<R> root) {
    Cx<R> r;
    r.re = sub_rn(x.re, root.re);
    r.im = sub_rn(x.im, root.im);
    return r;
}
// the one complex division: scaled (Smith)
template <typename R> RESP_HD Cx<R> cdiv(Cx<R> n, Cx<R> d) {
    Cx<R> q;
    const R ar = d.re < (R)0 ? -d.re : d.re, ai = d.im < (R)0 ? -d.im : d.im;
    if (ar >= ai) {
        const R r = div_rn(d.im, d.re), t = fma_rn(d.im, r, d.re);
        q.re = div_rn(fma_rn(n.im, r, n.re), t);
        q.im = div_rn(fma_rn(-n.re, r, n.im), t);
    } else {
        const R r = div_rn(d.re, d.im), t = fma_rn(d.re, r, d.im);
        q.re = div_rn(fma_rn(n.re, r, n.im), t);
        q.im = div_rn(fma_rn(n.im, r, -n.re), t);
    }
    return q;
}
// c: b0 b1 b2 a1 a2
template <typename R> RESP_HD Cx<R> biquad(const R* c, Cx<R> x) {
    Cx<R> t, u;
    t.re = fma_rn(c[0], x.re, c[1]);
    t.im = mul_rn(c[0], x.im);
    u.re = add_rn(x.re, c[3]);
    u.im = x.im;
    return cdiv(horner_step(t, x, c[2]), horner_step(u, x, c[4]));
}

// P(y) = sum_(k = lo .. hi-1) coef[k] y^(k - lo); an empty range gives zero
template <typename R, bool DERIV> RESP_HD Cx<R> poly_chunk(const R* coef, int64_t lo, int64_t hi, Cx<R> y) {
    Cx<R> acc;
    acc.re = (R)0;
    acc.im = (R)0;
    RESP_UNROLL8
    for (int64_t k = hi - 1; k >= lo; --k) {
        R v = coef[k];
        if (DERIV) v = mul_rn((R)k, v);
        acc = horner_step(acc, y, v);
    }
    return acc;
}
// y^(2^l) by l squarings.  A rounding of squaring s is doubled by every later one, so in the working type q = y^L would carry about L roundings of phase
// error and Horner over the chunks would multiply them by the chunk index (measured: 23 times the error of a serial chain at 4101 coefficients in
// chunks of 2048).  The squarings therefore run in double-word arithmetic (hi + lo, each an R; Dekker / Knuth sums, fma products),
// and q is rounded to R once, at the end.
template <typename R> struct DW { R hi, lo; };
template <typename R> RESP_HD DW<R> dw_fast_sum(R a, R b) {   // |a| >= |b| or a == 0
    DW<R> r;
    r.hi = add_rn(a, b);
    r.lo = sub_rn(b, sub_rn(r.hi, a));
    return r;
}
template <typename R> RESP_HD DW<R> dw_add(DW<R> a, DW<R> b) {
    const R s = add_rn(a.hi, b.hi), bb = sub_rn(s, a.hi);
    R e = add_rn(sub_rn(a.hi, sub_rn(s, bb)), sub_rn(b.hi, bb));
    e = add_rn(e, add_rn(a.lo, b.lo));
    return dw_fast_sum(s, e);
}
template <typename R> RESP_HD DW<R> dw_mul(DW<R> a, DW<R> b) {
    const R p = mul_rn(a.hi, b.hi);
    R e = fma_rn(a.hi, b.hi, -p);
    e = fma_rn(a.hi, b.lo, e);
    e = fma_rn(a.lo, b.hi, e);
    return dw_fast_sum(p, e);
}
template <typename R> RESP_HD Cx<R> pow2l(Cx<R> y, int l) {
    DW<R> re, im;
    re.hi = y.re;
    im.hi = y.im;
    re.lo = im.lo = (R)0;
    for (int s = 0; s < l; ++s) {
        DW<R> ii = dw_mul(im, im), ri = dw_mul(re, im);
        ii.hi = -ii.hi;
        ii.lo = -ii.lo;
        re = dw_add(dw_mul(re, re), ii);
        im.hi = add_rn(ri.hi, ri.hi);
        im.lo = add_rn(ri.lo, ri.lo);
    }
    y.re = add_rn(re.hi, re.lo);
    y.im = add_rn(im.hi, im.lo);
    return y;
}
// Horner over C chunk values stride apart, in q, from the highest
template <typename R> RESP_HD Cx<R> chunk_horner(const Cx<R>* p, int64_t stride, int64_t C, Cx<R> q) {
    Cx<R> acc = p[(C - 1) * stride];
    for (int64_t c = C - 2; c >= 0; --c) acc = horner_step_c(acc, q, p[c * stride]);
    return acc;
}
// g prod_k biquad_k(x), left to right from one
template <typename R> RESP_HD Cx<R> sections_value(const R* c, int K, R g, Cx<R> x) {
    Cx<R> acc;
    acc.re = (R)1;
    acc.im = (R)0;
    for (int k = 0; k < K; ++k) acc = cmul(acc, biquad(c + 5 * k, x));
    return scale(g, acc);
}
// (k prod (x - z_i)) / prod (x - p_i)
template <typename R> RESP_HD Cx<R> zpk_value(const Cx<R>* z, int64_t nz, const Cx<R>* p, int64_t np, R k, Cx<R> x) {
    Cx<R> a, b;
    a.re = b.re = (R)1;
    a.im = b.im = (R)0;
    for (int64_t i = 0; i < nz; ++i) a = cmul(a, sub_root(x, z[i]));
    for (int64_t i = 0; i < np; ++i) b = cmul(b, sub_root(x, p[i]));
    return cdiv(scale(k, a), b);
}

// ---- geometry: pure host arithmetic, the same on every machine
struct Geom {
    int64_t C = 1, L = MIN_L, workspace = 0;
    int log2L = 4;
};
inline int64_t next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
// ncoef: the longer of the two coefficient vectors (POLY); chunks: 0 = automatic, > 0 forced.  SECTIONS and ZPK are never cut.
inline Geom make_geometry(int form, bool dbl, int64_t ncoef, bool has_den, int64_t nw, int64_t chunks) {
    Geom g;
    if (form != FORM_POLY || ncoef < 1) return g;
    int64_t L = next_pow2(ncoef);
    if (chunks > 0) L = next_pow2((ncoef + chunks - 1) / chunks);
    else {
        const int64_t tiles = (nw + LANES - 1) / LANES;
        if (tiles > 0 && tiles < WAVES_TARGET && ncoef >= 2 * AUTO_MIN_L) {
            const int64_t want = (WAVES_TARGET + tiles - 1) / tiles;
            L = next_pow2((ncoef + want - 1) / want);
            if (L < AUTO_MIN_L) L = AUTO_MIN_L;
        }
    }
    if (L < MIN_L) L = MIN_L;
    g.L = L;
    g.log2L = 0;
    while (((int64_t)1 << g.log2L) < L) ++g.log2L;
    g.C = (ncoef + L - 1) / L;
    g.workspace = g.C > 1 ? (has_den ? 2 : 1) * g.C * nw * 2 * (dbl ? 8 : 4) : 0;
    return g;
}

}  // namespace resp
}  // namespace mdsp
