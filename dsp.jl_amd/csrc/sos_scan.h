// Biquad / SecondOrderSections filtering (Filters/filt.jl:35-51, :70-80) as a scan over runs of samples.
//
// Per sample and section, in the working type W, the reference's operations, each a function of its own (the library is compiled with
// -ffp-contract=on; a function per operation keeps host and device to the same roundings):
//
//     y  = fma(b0, x, s1)
//     s1 = fma(a1, -y, fma(b1, x, s2))
//     s2 = fma(b2, x, mul_rn(-a2, y))
//
// the output of a section is the input of the next, the output of the last is mul_rn(g, y) (SecondOrderSections) or y itself (Biquad).
//
// The recurrence is linear in (state, input): with z the 2K state values of the cascade (s1, s2 of section 0, s1, s2 of section 1, ...) a run of
// n samples maps z to A^n z + w, w the end state the run reaches from z = 0.  A is block lower triangular (a section sees only the sections in
// front of it) and so is every power.  That allows cutting a line: GIVEN THE STATE AT ITS FIRST SAMPLE, EVERY RUN OF SAMPLES IS COMPUTED BY THE
// SERIAL RECURRENCE ABOVE (walk_run); the scan (affine_add with rounded powers of A) only supplies start states.
//
// A line is cut into S segments of seglen samples, a segment into tiles of 64 runs of RUN consecutive samples.  Per tile: every run is walked from
// zero (run 0 from the state the tile starts in), a 64-wide Kogge-Stone scan v_l += A^(RUN 2^d) v_(l - 2^d), d = 0..5, turns the end states into the
// true ones, run l starts from v_(l-1) and is walked again, this time writing y; the state the walk of the tile's last sample ends in starts the next
// tile -- inside a segment the carry from tile to tile is the serial recurrence's own.  S > 1: (1) the zero-state end state of every segment,
// (2) the same scan over the S records of a line with A^(seglen 2^d), (3) apply.  The matrices are computed on the host in long double by repeated
// squaring and rounded once to W.
//
// Non-finite samples: in the reference a section never becomes finite again after a non-finite input (even with a1 = a2 = 0 the state takes
// fma(a1, -y, ...) = NaN), so the rest of the column is non-finite.  Here the state a run ends in is non-finite in every section from the first one
// hit, every row of M u sums over those entries (0 * NaN = NaN, Inf - Inf = NaN), and every later run starts non-finite: the same mask.
//
// Everything here is shared by the kernels (sos.hip) and the host emulation (mdsp_sos_emulate_host), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SOS_HD __host__ __device__ inline
#else
#define SOS_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define SOS_UNROLL _Pragma("unroll")
#else
#define SOS_UNROLL
#endif

namespace mdsp {
namespace sosscan {

constexpr int MAXK = 16;            // sections of the largest compiled cascade
constexpr int RUN = 16;             // P: consecutive samples per lane
constexpr int TILE = 64 * RUN;      // samples per tile
constexpr int LEVELS = 6;           // Kogge-Stone levels of a 64-wide scan

// compiled section counts; a cascade in between runs in the next one with its loops cut at K
inline int padded_sections(int64_t K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

// ---- one rounding per operation
SOS_HD float fma_rn(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return __builtin_fmaf(a, b, c);
#endif
}
SOS_HD double fma_rn(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);
#else
    return __builtin_fma(a, b, c);
#endif
}
SOS_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
SOS_HD double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}

// what a kernel needs of the filter, by value in its arguments: c[5 k ..] = b0 b1 b2 a1 a2 of section k
template <typename W, int KP> struct Coef {
    W c[5 * KP];
    W g;
    int K;          // sections in use, 1 <= K <= KP
    int has_gain;   // SecondOrderSections: the output is mul_rn(g, y); Biquad: y
};

// one sample through one section (filt.jl:44-46 / :74-76)
template <typename W> SOS_HD W section_step(const W* c, W x, W& s1, W& s2) {
    const W y = fma_rn(c[0], x, s1);
    s1 = fma_rn(c[3], -y, fma_rn(c[1], x, s2));
    s2 = fma_rn(c[2], x, mul_rn(-c[4], y));
    return y;
}

// The serial recurrence over the first `cnt` of the RUN samples in xs, from the state in st (2 KP values, 2 K in use), which it leaves at the
// run's end.  OUT = false: the state only (xs untouched); OUT = true: xs[t] becomes the output sample.
template <typename W, int KP, bool OUT> SOS_HD void walk_run(const Coef<W, KP>& f, W* xs, int cnt, W* st) {
    SOS_UNROLL
    for (int t = 0; t < RUN; ++t) {
        if (t < cnt) {
            W v = xs[t];
            SOS_UNROLL
            for (int k = 0; k < KP; ++k)
                if (k < f.K) v = section_step(f.c + 5 * k, v, st[2 * k], st[2 * k + 1]);
            if (OUT) xs[t] = f.has_gain ? mul_rn(f.g, v) : v;
        }
    }
}

// v <- v + M u, M one of the rounded powers of A, row-major with rows of 2 KP; row i: acc = v[i], then j ascending over the columns of the
// sections up to its own (the others are structurally zero), one fma each.
template <typename W, int KP> SOS_HD void affine_add(const W* M, int K, const W* u, W* v) {
    SOS_UNROLL
    for (int i = 0; i < 2 * KP; ++i) {
        if (i < 2 * K) {
            W acc = v[i];
            SOS_UNROLL
            for (int j = 0; j < 2 * (i / 2 + 1); ++j) acc = fma_rn(M[i * 2 * KP + j], u[j], acc);
            v[i] = acc;
        }
    }
}

// ---- geometry: pure host arithmetic, the same on every machine (256 compute units are assumed)
struct Geom {
    int64_t n = 0, ncols = 0, lines = 0, S = 1, seglen = 0, workspace = 0;
    int K = 1, KP = 1, cs = 1;   // cs: real lines per column (2 for a complex working type)
    int real_size = 4;
};
constexpr int64_t UNITS_TARGET = 256 * 8;   // (line, segment) wavefronts of an automatic cut
constexpr int64_t MINSEG_TILES = 4;         // shortest segment of an automatic cut, in tiles (a forced cut goes down to 1 sample)

inline Geom make_geometry(int64_t K, bool cplx, bool dbl, int64_t n, int64_t ncols, int64_t segments) {
    Geom g;
    g.K = (int)K;
    g.KP = padded_sections(K);
    g.cs = cplx ? 2 : 1;
    g.real_size = dbl ? 8 : 4;
    g.n = n;
    g.ncols = ncols;
    g.lines = ncols * g.cs;
    g.seglen = n;
    if (n == 0 || ncols == 0) return g;
    int64_t want = 1;
    if (segments > 0) want = segments < n ? segments : n;
    else if (g.lines < UNITS_TARGET) {
        want = (UNITS_TARGET + g.lines - 1) / g.lines;
        const int64_t cap = n / (MINSEG_TILES * TILE);
        want = want < cap ? want : cap;
        if (want < 1) want = 1;
    }
    g.seglen = (n + want - 1) / want;
    if (segments <= 0 && want > 1) g.seglen = (g.seglen + TILE - 1) / TILE * TILE;   // an automatic cut falls on tile boundaries
    g.S = (n + g.seglen - 1) / g.seglen;
    g.workspace = g.S > 1 ? g.lines * g.S * 2 * g.K * g.real_size : 0;
    return g;
}

// ---- the carry matrices.  A from the coefficients as the kernels use them (already rounded to W, passed as long double), its powers by repeated
// squaring in long double.
struct LMat {
    int n = 0;
    std::vector<long double> a;   // n x n, row-major
    long double& at(int i, int j) { return a[(size_t)i * n + j]; }
    long double at(int i, int j) const { return a[(size_t)i * n + j]; }
};
inline LMat state_matrix(const long double* c, int K) {
    LMat A;
    A.n = 2 * K;
    A.a.assign((size_t)A.n * A.n, 0.0L);
    std::vector<long double> st((size_t)A.n);
    for (int col = 0; col < A.n; ++col) {
        for (int i = 0; i < A.n; ++i) st[i] = i == col ? 1.0L : 0.0L;
        long double v = 0.0L;   // x = 0: the state's own evolution
        for (int k = 0; k < K; ++k) {
            const long double *q = c + 5 * k, y = q[0] * v + st[2 * k];
            const long double s1 = -q[3] * y + (q[1] * v + st[2 * k + 1]), s2 = q[2] * v - q[4] * y;
            st[2 * k] = s1;
            st[2 * k + 1] = s2;
            v = y;
        }
        for (int i = 0; i < A.n; ++i) A.at(i, col) = st[i];
    }
    return A;
}
inline LMat matmul(const LMat& x, const LMat& y) {
    LMat r;
    r.n = x.n;
    r.a.assign((size_t)r.n * r.n, 0.0L);
    for (int i = 0; i < r.n; ++i)
        for (int k = 0; k < r.n; ++k) {
            const long double xik = x.at(i, k);
            if (xik == 0.0L) continue;
            for (int j = 0; j < r.n; ++j) r.at(i, j) += xik * y.at(k, j);
        }
    return r;
}
inline LMat matpow(const LMat& A, int64_t e) {
    LMat r;
    r.n = A.n;
    r.a.assign((size_t)r.n * r.n, 0.0L);
    for (int i = 0; i < r.n; ++i) r.at(i, i) = 1.0L;
    LMat b = A;
    while (e > 0) {
        if (e & 1) r = matmul(r, b);
        e >>= 1;
        if (e) b = matmul(b, b);
    }
    return r;
}
// A^(base 2^d), d = 0 .. LEVELS-1, rounded once to W into out[d (2 KP)^2 ..] (rows of 2 KP, the padding zero).  false: an entry is not finite in W.
template <typename W> inline bool power_ladder(const LMat& A, int64_t base, int KP, W* out) {
    LMat p = matpow(A, base);
    const int ld = 2 * KP;
    for (int d = 0; d < LEVELS; ++d) {
        W* m = out + (size_t)d * ld * ld;
        for (int i = 0; i < ld * ld; ++i) m[i] = (W)0;
        for (int i = 0; i < A.n; ++i)
            for (int j = 0; j < A.n; ++j) {
                const W w = (W)p.at(i, j);
                if (!std::isfinite(w)) return false;
                m[i * ld + j] = w;
            }
        if (d + 1 < LEVELS) p = matmul(p, p);
    }
    return true;
}

// ---- host emulation of a 64-wide scan step by step as the wavefront does it: every lane reads its neighbour's value of BEFORE the level
template <typename W, int KP> inline void scan64_host(const W* mats, int K, W (*v)[2 * KP]) {
    W u[64][2 * KP];
    for (int d = 0; d < LEVELS; ++d) {
        const int off = 1 << d;
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 2 * KP; ++i) u[l][i] = v[l][i];
        for (int l = off; l < 64; ++l) affine_add<W, KP>(mats + (size_t)d * 4 * KP * KP, K, u[l - off], v[l]);
    }
}

// One (line, segment) on the host: samples j0 .. j1-1 of the line at x (element stride inc; reverse: sample j is element n-1-j), tile by tile.
// z: the 2 K state values at j0 on entry, at j1 on return.  y == nullptr: the state only.
template <typename W, int KP>
inline void unit_host(const Coef<W, KP>& f, const W* tilemats, const W* x, W* y, int64_t inc_x, int64_t inc_y, int64_t n, int reverse, int64_t j0, int64_t j1, W* z) {
    std::vector<W> buf((size_t)TILE);
    W(*v)[2 * KP] = new W[64][2 * KP];
    for (int64_t t0 = j0; t0 < j1; t0 += TILE) {
        const int64_t cnt = j1 - t0 < TILE ? j1 - t0 : TILE;
        for (int64_t i = 0; i < cnt; ++i) buf[(size_t)i] = x[(reverse ? n - 1 - (t0 + i) : t0 + i) * inc_x];   // the whole tile is read before any of it is written
        for (int l = 0; l < 64; ++l) {
            for (int i = 0; i < 2 * KP; ++i) v[l][i] = l == 0 && i < 2 * f.K ? z[i] : (W)0;
            const int64_t c = cnt - (int64_t)l * RUN;
            walk_run<W, KP, false>(f, &buf[(size_t)(c > 0 ? l * RUN : 0)], (int)(c < 0 ? 0 : c > RUN ? RUN : c), v[l]);
        }
        scan64_host<W, KP>(tilemats, f.K, v);
        const int last = (int)((cnt - 1) / RUN);
        W st[2 * KP], zn[2 * KP];
        for (int l = 0; l <= last; ++l) {
            for (int i = 0; i < 2 * KP; ++i) st[i] = l == 0 ? (i < 2 * f.K ? z[i] : (W)0) : v[l - 1][i];
            const int64_t c = cnt - (int64_t)l * RUN;
            walk_run<W, KP, true>(f, &buf[(size_t)l * RUN], (int)(c > RUN ? RUN : c), st);
            if (l == last)
                for (int i = 0; i < 2 * KP; ++i) zn[i] = st[i];
        }
        for (int i = 0; i < 2 * f.K; ++i) z[i] = zn[i];
        if (y)
            for (int64_t i = 0; i < cnt; ++i) y[(reverse ? n - 1 - (t0 + i) : t0 + i) * inc_y] = buf[(size_t)i];
    }
    delete[] v;
}

// step 2 for one line on the host: rec holds S records of 2 K values, the zero-state end states; on return the state at each segment's first sample.
// z0: the state at the line's first sample.  64 records at a time, as the wavefront does it.
template <typename W, int KP> inline void carries_host(const W* segmats, int K, W* rec, int64_t S, const W* z0) {
    W(*v)[2 * KP] = new W[64][2 * KP];
    W r[2 * KP];
    for (int i = 0; i < 2 * KP; ++i) r[i] = i < 2 * K ? z0[i] : (W)0;
    for (int64_t s0 = 0; s0 < S; s0 += 64) {
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 2 * KP; ++i) v[l][i] = s0 + l < S && i < 2 * K ? rec[(s0 + l) * 2 * K + i] : (W)0;
        affine_add<W, KP>(segmats, K, r, v[0]);
        scan64_host<W, KP>(segmats, K, v);
        for (int l = 0; l < 64 && s0 + l < S; ++l)
            for (int i = 0; i < 2 * K; ++i) rec[(s0 + l) * 2 * K + i] = l == 0 ? r[i] : v[l - 1][i];
        for (int i = 0; i < 2 * KP; ++i) r[i] = v[63][i];
    }
    delete[] v;
}

}  // namespace sosscan
}  // namespace mdsp
