// One pass of the Quinn & Fernandes / Quinn iterations (src/estimation.jl:157-220) as a scan over runs of samples whose sink is a handful of sums:
// the filtered signal xi is never stored.
//
// State and recurrence are Float64 whatever the signal's type (the reference forms every xi[t] in Float64 from a Float64 alpha and only rounds the stored
// value to the element type).  Samples are loaded as Float32, Float64, ComplexF32 or ComplexF64, converted exactly and the mean removed at the load:
//     d_t = add_rn((double)x_t, -mu)                       one rounding (both parts of a complex sample); no mean-removed copy is written
// Every operation below is a function of its own (the library is compiled with -ffp-contract=on), t counts from 1 as in the reference, xi_0 = xi_-1 = 0.
//
//   REAL pass, given alpha (:176-182):
//     xi_t  = add_rn(d_t, fma_rn(alpha, xi_(t-1), -xi_(t-2)))                 for every t.  At t = 2 this is one rounding more than :176's muladd.
//     num  += mul_rn(add_rn(xi_t, xi_(t-2)), xi_(t-1))                        t = 3 .. N
//     den  += mul_rn(xi_t, xi_t)                                              t = 1 .. N-1
//     record {num, den, xi_1, xi_2}; the host forms beta = (xi_2 / xi_1 + num) / den.
//   COMPLEX pass, given c = cis(omega) (:205-212), z = (re, im):
//     S.re += fma_rn(d.re, xi.re, mul_rn(d.im, xi.im)),  S.im += fma_rn(d.im, xi.re, -mul_rn(d.re, xi.im))      d_t conj(xi_(t-1)),  t = 2 .. N
//     xi_t  = (add_rn(d.re, fma_rn(c.re, xi.re, -mul_rn(c.im, xi.im))), add_rn(d.im, fma_rn(c.re, xi.im, mul_rn(c.im, xi.re))))
//     den  += fma_rn(xi_t.re, xi_t.re, mul_rn(xi_t.im, xi_t.im))              t = 1 .. N-1
//     record {S.re, S.im, den}.
//
// Both recurrences are linear in (state, input): a run of m samples maps the state z to A^m z + w, w the state the run reaches from zero, with
// A = [alpha -1; 1 0] on (xi_(t-1), xi_(t-2)), or A = c on the complex xi_(t-1).  The geometry is that of sos_scan.h: a line is cut into S segments of
// seglen samples, a segment into tiles of 64 runs of RUN consecutive samples.  Per tile every lane walks its run from zero (run 0 from the state the tile
// starts in), a 64-wide Kogge-Stone scan v_l += A^(RUN 2^d) v_(l - 2^d), d = 0..5, turns the end states into the true ones, run l starts from v_(l-1) and
// is walked AGAIN BY THE SERIAL RECURRENCE ABOVE, this time adding its terms; the state the walk of the tile's last sample ends in starts the next tile.
// S > 1: (1) the zero-state end state of every segment, (2) the same scan over the S records with A^(seglen 2^d), (3) the summing pass from the true
// start states, one partial per segment, (4) a finish over the partials.  The poles lie ON the unit circle: a wrong start state never decays, so the
// accuracy of a pass is that of the powers, which the host computes in long double by repeated squaring and rounds once.
//
// ORDER OF ADDITIONS.  A lane adds the terms of its runs in ascending t, tile after tile, into its own accumulators (from zero); at the segment's end
// the 64 accumulators are folded as fold64 of reduce_op.h does (for off = 32, 16, .., 1: acc[l] += acc[l + off], l < off); S > 1: lane l of the
// finish adds the partials l, l + 64, .. in ascending order (finish_walk), then the same fold.  affine_add: acc = v[i], then one fma per column, ascending.
// No atomics, no flags, nothing waits for another workgroup.
//
// Everything here is shared by the kernels (estimation.hip) and the host emulation (mdsp_quinn_pass_emulate_host), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "reduce_op.h"

#if defined(__HIPCC__)
#define QUINN_HD __host__ __device__ inline
#else
#define QUINN_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define QUINN_UNROLL _Pragma("unroll")
#else
#define QUINN_UNROLL
#endif

namespace mdsp {
namespace quinnscan {

using reduceop::add_rn;
using reduceop::c32;
using reduceop::c64;
using reduceop::mul_rn;

constexpr int RUN = 16;             // P: consecutive samples per lane
constexpr int TILE = 64 * RUN;      // samples per tile
constexpr int LEVELS = 6;           // Kogge-Stone levels of a 64-wide scan
constexpr int NSTATE = 2;           // doubles of a state: (xi_(t-1), xi_(t-2)) or (re, im)

QUINN_HD double fma_rn(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);
#else
    return __builtin_fma(a, b, c);
#endif
}

// CPLX: the form of the pass.  NMAT doubles per power of A, NSUM sums, NREC doubles of the record.
template <bool CPLX> struct Form {
    static constexpr int NMAT = CPLX ? 2 : 4;
    static constexpr int NSUM = CPLX ? 3 : 2;
    static constexpr int NREC = CPLX ? 3 : 4;
};

// the partial sums as an operator for finish_walk / fold64 of reduce_op.h
template <int N> struct Sums { double s[N]; };
template <int N> struct OpSums {
    using Acc = Sums<N>;
    QUINN_HD static Acc identity() {
        Acc a;
        for (int i = 0; i < N; ++i) a.s[i] = 0.0;
        return a;
    }
    QUINN_HD static Acc combine(Acc a, Acc b, const reduceop::Params&) {
        for (int i = 0; i < N; ++i) a.s[i] = add_rn(a.s[i], b.s[i]);
        return a;
    }
};

// what a kernel needs of the iteration, by value in its arguments (alpha changes every iteration: nothing is copied to the device)
template <bool CPLX> struct Pass {
    double p[2];                                  // alpha, or (cos omega, sin omega)
    double mu[2];                                 // the mean (re, im)
    double tile[LEVELS * Form<CPLX>::NMAT];       // A^(RUN 2^d), row-major
    double seg[LEVELS * Form<CPLX>::NMAT];        // A^(seglen 2^d) (S > 1)
};

QUINN_HD void sample(float x, const double* mu, double* d) { d[0] = add_rn((double)x, -mu[0]); }
QUINN_HD void sample(double x, const double* mu, double* d) { d[0] = add_rn(x, -mu[0]); }
QUINN_HD void sample(c32 x, const double* mu, double* d) {
    d[0] = add_rn((double)x.re, -mu[0]);
    d[1] = add_rn((double)x.im, -mu[1]);
}
QUINN_HD void sample(c64 x, const double* mu, double* d) {
    d[0] = add_rn(x.re, -mu[0]);
    d[1] = add_rn(x.im, -mu[1]);
}

// The serial recurrence over the first `cnt` of the RUN samples in xs -- samples j .. j + cnt - 1 of the line, 0-based, of n -- from the state in st, which it
// leaves at the run's end.  SUM: the terms go to acc[NSUM], and xi_1, xi_2 of the real form (j = 0, 1) to first[0], first[1], stored by whoever walks them.
template <bool CPLX, bool SUM, typename T>
QUINN_HD void walk_run(const double* p, const double* mu, const T* xs, int cnt, int64_t j, int64_t n, double* st, double* acc, double* first) {
    QUINN_UNROLL
    for (int t = 0; t < RUN; ++t) {
        if (t < cnt) {
            double d[2];
            sample(xs[t], mu, d);
            const int64_t jt = j + t;
            if constexpr (!CPLX) {
                const double xi = add_rn(d[0], fma_rn(p[0], st[0], -st[1]));
                if constexpr (SUM) {
                    if (jt >= 2) acc[0] = add_rn(acc[0], mul_rn(add_rn(xi, st[1]), st[0]));
                    if (jt < n - 1) acc[1] = add_rn(acc[1], mul_rn(xi, xi));
                    if (jt < 2) first[jt] = xi;
                }
                st[1] = st[0];
                st[0] = xi;
            } else {
                if constexpr (SUM) {
                    if (jt >= 1) {
                        acc[0] = add_rn(acc[0], fma_rn(d[0], st[0], mul_rn(d[1], st[1])));
                        acc[1] = add_rn(acc[1], fma_rn(d[1], st[0], -mul_rn(d[0], st[1])));
                    }
                }
                const double re = add_rn(d[0], fma_rn(p[0], st[0], -mul_rn(p[1], st[1])));
                const double im = add_rn(d[1], fma_rn(p[0], st[1], mul_rn(p[1], st[0])));
                if constexpr (SUM) {
                    if (jt < n - 1) acc[2] = add_rn(acc[2], fma_rn(re, re, mul_rn(im, im)));
                }
                st[0] = re;
                st[1] = im;
            }
        }
    }
}

// v <- v + M u, M one of the rounded powers of A
template <bool CPLX> QUINN_HD void affine_add(const double* M, const double* u, double* v) {
    if constexpr (!CPLX) {
        v[0] = fma_rn(M[1], u[1], fma_rn(M[0], u[0], v[0]));
        v[1] = fma_rn(M[3], u[1], fma_rn(M[2], u[0], v[1]));
    } else {
        v[0] = fma_rn(-M[1], u[1], fma_rn(M[0], u[0], v[0]));
        v[1] = fma_rn(M[1], u[0], fma_rn(M[0], u[1], v[1]));
    }
}

// ---- geometry: pure host arithmetic, the same on every machine (256 compute units are assumed); the rule of sos_scan.h for one line
struct Geom {
    int64_t n = 0, S = 1, seglen = 0, workspace = 0;
    bool cplx = false;
};
constexpr int64_t UNITS_TARGET = 256 * 8;   // segment wavefronts of an automatic cut
constexpr int64_t MINSEG_TILES = 4;         // shortest segment of an automatic cut, in tiles (a forced cut goes down to 1 sample)

inline Geom make_geometry(bool cplx, int64_t n, int64_t segments) {
    Geom g;
    g.n = n;
    g.cplx = cplx;
    int64_t want = 1;
    if (segments > 0) want = segments < n ? segments : n;
    else {
        want = UNITS_TARGET;
        const int64_t cap = n / (MINSEG_TILES * TILE);
        want = want < cap ? want : cap;
        if (want < 1) want = 1;
    }
    g.seglen = (n + want - 1) / want;
    if (segments <= 0 && want > 1) g.seglen = (g.seglen + TILE - 1) / TILE * TILE;   // an automatic cut falls on tile boundaries
    g.S = (n + g.seglen - 1) / g.seglen;
    // S > 1: a state and a partial per segment
    g.workspace = g.S > 1 ? g.S * 8 * (NSTATE + (cplx ? Form<true>::NSUM : Form<false>::NSUM)) : 0;
    return g;
}

// ---- the powers of A: long double, repeated squaring, rounded once.  false: an entry is not finite in Float64.
struct LM {
    long double a[4];   // real form: 2 x 2 row-major; complex form: (re, im, -, -)
};
template <bool CPLX> inline LM lm_mul(const LM& x, const LM& y) {
    LM r{};
    if constexpr (!CPLX) {
        r.a[0] = x.a[0] * y.a[0] + x.a[1] * y.a[2];
        r.a[1] = x.a[0] * y.a[1] + x.a[1] * y.a[3];
        r.a[2] = x.a[2] * y.a[0] + x.a[3] * y.a[2];
        r.a[3] = x.a[2] * y.a[1] + x.a[3] * y.a[3];
    } else {
        r.a[0] = x.a[0] * y.a[0] - x.a[1] * y.a[1];
        r.a[1] = x.a[0] * y.a[1] + x.a[1] * y.a[0];
    }
    return r;
}
template <bool CPLX> inline LM lm_pow(LM b, int64_t e) {
    LM r{};
    r.a[0] = 1.0L;
    if (!CPLX) r.a[3] = 1.0L;
    while (e > 0) {
        if (e & 1) r = lm_mul<CPLX>(r, b);
        e >>= 1;
        if (e) b = lm_mul<CPLX>(b, b);
    }
    return r;
}
// A^(base 2^d), d = 0 .. LEVELS-1, into out[d NMAT ..]; p: alpha or (cos, sin) as the kernels use them
template <bool CPLX> inline bool power_ladder(const double* p, int64_t base, double* out) {
    LM A{};
    if constexpr (!CPLX) {
        A.a[0] = (long double)p[0];
        A.a[1] = -1.0L;
        A.a[2] = 1.0L;
    } else {
        A.a[0] = (long double)p[0];
        A.a[1] = (long double)p[1];
    }
    LM q = lm_pow<CPLX>(A, base);
    for (int d = 0; d < LEVELS; ++d) {
        for (int i = 0; i < Form<CPLX>::NMAT; ++i) {
            const double w = (double)q.a[i];
            if (!std::isfinite(w)) return false;
            out[d * Form<CPLX>::NMAT + i] = w;
        }
        if (d + 1 < LEVELS) q = lm_mul<CPLX>(q, q);
    }
    return true;
}

// ---- host emulation of a 64-wide scan step by step as the wavefront does it: every lane reads its neighbour's value of BEFORE the level
template <bool CPLX> inline void scan64_host(const double* mats, double (*v)[NSTATE]) {
    double u[64][NSTATE];
    for (int d = 0; d < LEVELS; ++d) {
        const int off = 1 << d;
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < NSTATE; ++i) u[l][i] = v[l][i];
        for (int l = off; l < 64; ++l) affine_add<CPLX>(mats + d * Form<CPLX>::NMAT, u[l - off], v[l]);
    }
}

// One segment on the host: samples j0 .. j1-1 of the line at x, tile by tile.  z: the state at j0 on entry, at j1 on return.  lanes == nullptr: the state
// only; else the 64 lanes' accumulators (NSUM each, zero on entry) take the terms, and first (real form) xi_1, xi_2.
template <bool CPLX, typename T>
inline void unit_host(const Pass<CPLX>& ps, const T* x, int64_t n, int64_t j0, int64_t j1, double* z, double (*lanes)[3], double* first) {
    double v[64][NSTATE];
    for (int64_t t0 = j0; t0 < j1; t0 += TILE) {
        const int64_t cnt = j1 - t0 < TILE ? j1 - t0 : TILE;
        auto mine = [&](int l) {
            const int64_t c = cnt - (int64_t)l * RUN;
            return (int)(c < 0 ? 0 : c > RUN ? RUN : c);
        };
        for (int l = 0; l < 64; ++l) {
            for (int i = 0; i < NSTATE; ++i) v[l][i] = l == 0 ? z[i] : 0.0;
            walk_run<CPLX, false, T>(ps.p, ps.mu, x + t0 + (mine(l) > 0 ? l * RUN : 0), mine(l), t0 + l * RUN, n, v[l], nullptr, nullptr);
        }
        scan64_host<CPLX>(ps.tile, v);
        const int last = (int)((cnt - 1) / RUN);
        double st[NSTATE];
        for (int l = 0; l <= last; ++l) {
            for (int i = 0; i < NSTATE; ++i) st[i] = l == 0 ? z[i] : v[l - 1][i];
            if (lanes) walk_run<CPLX, true, T>(ps.p, ps.mu, x + t0 + l * RUN, mine(l), t0 + l * RUN, n, st, lanes[l], first);
            else walk_run<CPLX, false, T>(ps.p, ps.mu, x + t0 + l * RUN, mine(l), t0 + l * RUN, n, st, nullptr, nullptr);
        }
        for (int i = 0; i < NSTATE; ++i) z[i] = st[i];   // (of run `last`)
    }
}

// step 2 on the host: rec holds S zero-state end states; on return the state at each segment's first sample (the line starts from zero).  64 at a time.
template <bool CPLX> inline void carries_host(const double* segmats, double* rec, int64_t S) {
    double v[64][NSTATE];
    double r[NSTATE] = {0.0, 0.0};
    for (int64_t s0 = 0; s0 < S; s0 += 64) {
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < NSTATE; ++i) v[l][i] = s0 + l < S ? rec[(s0 + l) * NSTATE + i] : 0.0;
        affine_add<CPLX>(segmats, r, v[0]);
        scan64_host<CPLX>(segmats, v);
        for (int l = 0; l < 64 && s0 + l < S; ++l)
            for (int i = 0; i < NSTATE; ++i) rec[(s0 + l) * NSTATE + i] = l == 0 ? r[i] : v[l - 1][i];
        for (int i = 0; i < NSTATE; ++i) r[i] = v[63][i];
    }
}

// the whole pass on the host; out: the record (NREC doubles)
template <bool CPLX, typename T> inline void emulate(const Pass<CPLX>& ps, const Geom& g, const T* x, double* out) {
    constexpr int NS = Form<CPLX>::NSUM;
    using Op = OpSums<NS>;
    const reduceop::Params prm{0.0, 0};
    std::vector<double> states((size_t)(g.S * NSTATE), 0.0);
    std::vector<typename Op::Acc> part((size_t)g.S);
    if (g.S > 1) {
        for (int64_t s = 0; s < g.S; ++s) unit_host<CPLX, T>(ps, x, g.n, s * g.seglen, std::min(g.n, (s + 1) * g.seglen), &states[(size_t)(s * NSTATE)], nullptr, nullptr);
        carries_host<CPLX>(ps.seg, states.data(), g.S);
    }
    for (int64_t s = 0; s < g.S; ++s) {
        double lanes[64][3] = {};
        unit_host<CPLX, T>(ps, x, g.n, s * g.seglen, std::min(g.n, (s + 1) * g.seglen), &states[(size_t)(s * NSTATE)], lanes, out + 2);
        typename Op::Acc a[64];
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < NS; ++i) a[l].s[i] = lanes[l][i];
        part[(size_t)s] = reduceop::fold64<Op>(a, prm);
    }
    typename Op::Acc res = part[0];
    if (g.S > 1) {
        typename Op::Acc a[64];
        for (int l = 0; l < 64; ++l) a[l] = reduceop::finish_walk<Op>(part.data(), g.S, l, prm);
        res = reduceop::fold64<Op>(a, prm);
    }
    for (int i = 0; i < NS; ++i) out[i] = res.s[i];
}

}  // namespace quinnscan
}  // namespace mdsp
