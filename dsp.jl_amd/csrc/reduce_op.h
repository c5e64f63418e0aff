// Deterministic reductions along one dimension of an (inner, len, outer) array -- element (i, j, o) at i + inner (j + len o), reduced along j -- in the
// "store, then sum" form: every partial result is stored by exactly one lane and summed later in a fixed order; no float atomics, nothing waits for
// another workgroup, and a result is the same bits exec after exec.  Three operators (src/util.jl:186-220, :336-347):
//
//   SUMABS2     sum |x_j|^2 in Float64.  Float32 / ComplexF32 terms are formed in Float64 (each product exact there); Float64 terms are rounded as the
//               reference's abs2 does (ComplexF64: re*re + im*im, three roundings, no FMA contraction).
//   SUMABS2_W   complex bins X_k: the two Float64 sums  sum p_k (k step)  and  sum p_k,  p_k = abs2(X_k) rounded in the element's real type
//               (abs2.(rfft(x))), k step and the product rounded in Float64 (fs/len .* (0:npoints), pxx .* freqrg).
//   ABSARGMAX   a real line and a centre index: the index of the largest |x_j|; at equal magnitude the index nearer to the centre, at equal distance
//               the smaller index (maximum / findall / argmin of util.jl:338-346).  The rule is a total order, so the operator is associative and
//               commutative and the result does not depend on the cut.  NaN samples do not compete and raise a flag.
//
// ORDER OF ADDITIONS.  A line is cut into S segments of seglen (the last one ragged); a unit is (line, segment).
//   contiguous route (inner == 1): 64 lanes per unit.  Tiles of 64 x V elements (V = 16 bytes / element) stand on 16-byte boundaries of the ADDRESS:
//       with a = (address of the segment's first element / element size) mod V, tile t starts at element j0 - a + 64 V t, lane l owns the V elements
//       from j0 - a + (64 t + l) V on and adds those inside [j0, j1) to its accumulator in ascending order, tile after tile.  Then the 64 accumulators
//       are folded: for off = 32, 16, .., 1: acc[l] = acc[l] (+) acc[l + off] for l < off.  The result depends on `a` and on nothing else of the address.
//   strided route (inner > 1): a lane per (i, o, segment) adds its elements in ascending j.
//   finish (S > 1): 64 lanes per line; lane l adds the partials l, l + 64, .. in ascending order, then the same fold.
// Every addition is one IEEE Float64 add (the library is built with -ffp-contract=on; each operation below is a function of its own, the device forms
// are __dadd_rn / __dmul_rn / __fadd_rn / __fmul_rn).  `depth` of a geometry bounds the number of additions any term passes through.
//
// Everything here is shared by the kernels (reduce.hip) and the host emulation (mdsp_reduce_emulate), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define REDUCE_HD __host__ __device__ inline
#else
#define REDUCE_HD inline
#endif

namespace mdsp {
namespace reduceop {

enum : int { OP_SUMABS2 = 0, OP_SUMABS2_W = 1, OP_ABSARGMAX = 2 };
enum : int { ROUTE_CONTIGUOUS = 0, ROUTE_STRIDED = 1 };

template <typename R> struct cpx { R re, im; };
using c32 = cpx<float>;
using c64 = cpx<double>;

struct Params {
    double step;      // SUMABS2_W: fs / len
    int64_t centre;   // ABSARGMAX
};

// ---- one rounding per operation
REDUCE_HD double add_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
REDUCE_HD double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
REDUCE_HD float add_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
REDUCE_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

// |x|^2 as SUMABS2 adds it
REDUCE_HD double abs2_f64(float x) { return mul_rn((double)x, (double)x); }
REDUCE_HD double abs2_f64(double x) { return mul_rn(x, x); }
REDUCE_HD double abs2_f64(c32 x) { return add_rn(mul_rn((double)x.re, (double)x.re), mul_rn((double)x.im, (double)x.im)); }
REDUCE_HD double abs2_f64(c64 x) { return add_rn(mul_rn(x.re, x.re), mul_rn(x.im, x.im)); }
// abs2 rounded in the element's real type, as SUMABS2_W takes it
REDUCE_HD double abs2_own(c32 x) { return (double)add_rn(mul_rn(x.re, x.re), mul_rn(x.im, x.im)); }
REDUCE_HD double abs2_own(c64 x) { return add_rn(mul_rn(x.re, x.re), mul_rn(x.im, x.im)); }

// ---- the operators: Acc, identity, term(element, index along the line), combine (a before b; all three are commutative)
struct Sum1 { double s; };
struct Sum2 { double num, den; };
struct Arg {
    double a;       // |x| of the candidate; -1: none yet
    int64_t idx;    // its index along the line; -1: none
    int64_t nan;    // 1: a NaN was seen
};

struct OpSumAbs2 {
    using Acc = Sum1;
    static constexpr int NOUT = 1;   // 8-byte words of a line's result
    REDUCE_HD static Acc identity() { return Acc{0.0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t, const Params&) { return Acc{abs2_f64(x)}; }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params&) { return Acc{add_rn(a.s, b.s)}; }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) { static_cast<double*>(out)[line] = a.s; }
};
struct OpSumAbs2W {
    using Acc = Sum2;
    static constexpr int NOUT = 2;
    REDUCE_HD static Acc identity() { return Acc{0.0, 0.0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t k, const Params& p) {
        const double pk = abs2_own(x);
        return Acc{mul_rn(pk, mul_rn(p.step, (double)k)), pk};
    }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params&) { return Acc{add_rn(a.num, b.num), add_rn(a.den, b.den)}; }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) {
        static_cast<double*>(out)[2 * line] = a.num;
        static_cast<double*>(out)[2 * line + 1] = a.den;
    }
};
struct OpAbsArgmax {
    using Acc = Arg;
    static constexpr int NOUT = 2;
    REDUCE_HD static Acc identity() { return Acc{-1.0, -1, 0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t j, const Params&) {
        const double v = (double)x;
        if (v != v) return Acc{-1.0, -1, 1};
        return Acc{v < 0 ? -v : v, j, 0};
    }
    REDUCE_HD static bool nearer(int64_t i, int64_t k, int64_t c) {
        const int64_t di = i > c ? i - c : c - i, dk = k > c ? k - c : c - k;
        return di < dk || (di == dk && i < k);
    }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params& p) {
        const bool takeb = b.a > a.a || (b.a == a.a && nearer(b.idx, a.idx, p.centre));
        return Acc{takeb ? b.a : a.a, takeb ? b.idx : a.idx, a.nan | b.nan};
    }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) {   // the record (index, flag): two ordinary 8-byte stores
        static_cast<int64_t*>(out)[2 * line] = a.idx;
        static_cast<int64_t*>(out)[2 * line + 1] = a.nan;
    }
};

// ---- geometry: pure host arithmetic, independent of the device (256 compute units assumed, as for unwrap)
struct Geom {
    int route = ROUTE_CONTIGUOUS;
    int64_t inner = 0, len = 0, outer = 0, lines = 0, S = 1, seglen = 0, workspace = 0, depth = 0;
};
constexpr int LANES = 64;                              // lanes of a unit of the contiguous route and of a line of the finish
constexpr int TILES_AHEAD = 4;                         // tiles loaded before the first of them is added (loads in flight; the order does not change)
constexpr int64_t WAVES_TARGET = 256 * 32;             // contiguous route: a wavefront per unit, 32 resident per compute unit
constexpr int64_t LANES_TARGET = WAVES_TARGET * 64;    // strided route: a lane per unit
constexpr int64_t MINSEG_CONTIGUOUS = 8192, MINSEG_STRIDED = 256;   // shortest segments of an automatic cut (a forced one goes down to 1)

inline int64_t acc_bytes(int op) { return op == OP_SUMABS2 ? (int64_t)sizeof(Sum1) : op == OP_SUMABS2_W ? (int64_t)sizeof(Sum2) : (int64_t)sizeof(Arg); }

// elem_bytes: 4, 8 or 16; is_complex adds the addition inside a term (re*re + im*im)
inline Geom make_geometry(int64_t inner, int64_t len, int64_t outer, int op, int64_t elem_bytes, bool is_complex, int64_t segments) {
    Geom g;
    g.route = inner == 1 ? ROUTE_CONTIGUOUS : ROUTE_STRIDED;
    g.inner = inner;
    g.len = len;
    g.outer = outer;
    g.lines = inner * outer;
    g.seglen = len;
    if (g.lines == 0) return g;
    int64_t want = 1;
    if (len == 0) want = 1;   // one empty segment per line: the result is the identity
    else if (segments > 0) want = segments < len ? segments : len;
    else {
        const int64_t target = g.route == ROUTE_CONTIGUOUS ? WAVES_TARGET : LANES_TARGET;
        const int64_t minseg = g.route == ROUTE_CONTIGUOUS ? MINSEG_CONTIGUOUS : MINSEG_STRIDED;
        if (g.lines < target) {
            want = (target + g.lines - 1) / g.lines;
            const int64_t cap = len / minseg;
            want = want < cap ? want : cap;
            if (want < 1) want = 1;
        }
    }
    g.seglen = (len + want - 1) / want;
    g.S = len == 0 ? 1 : (len + g.seglen - 1) / g.seglen;   // no empty segment (but the one of an empty line)
    g.workspace = g.S > 1 ? g.lines * g.S * acc_bytes(op) : 0;
    const int64_t V = 16 / elem_bytes;
    // contiguous: a lane owns V elements of each of the tiles that cover a - 1 + seglen elements at worst (a <= V - 1), then six folds
    const int64_t walk = g.route == ROUTE_CONTIGUOUS ? V * ((g.seglen + V - 1 + LANES * V - 1) / (LANES * V)) + 6 : g.seglen;
    g.depth = walk + (g.S > 1 ? (g.S + LANES - 1) / LANES + 6 : 0) + (is_complex ? 1 : 0);
    return g;
}

// ---- the walk of one lane of a contiguous unit.  `ld.vec(p, v)` loads the V elements from element p on (a 16-byte boundary on the device),
// `ld.one(e)` element e; nothing outside [j0, j1) is touched.  *chain (host only) counts the additions.
template <typename T> struct HostLoad {
    const T* m;
    static constexpr int V = 16 / (int)sizeof(T);
    REDUCE_HD void vec(int64_t p, T* v) const {
        for (int k = 0; k < V; ++k) v[k] = m[p + k];
    }
    REDUCE_HD T one(int64_t e) const { return m[e]; }
};

template <typename Op, typename T, typename Load>
REDUCE_HD typename Op::Acc lane_walk(const Load& ld, int64_t j0, int64_t j1, int64_t a, int lane, const Params& prm, int64_t* chain = nullptr) {
    constexpr int V = 16 / (int)sizeof(T);
    typename Op::Acc acc = Op::identity();
    for (int64_t p0 = j0 - a; p0 < j1; p0 += (int64_t)LANES * V * TILES_AHEAD) {
        T v[TILES_AHEAD][V];
        bool full[TILES_AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int t = 0; t < TILES_AHEAD; ++t) {
            const int64_t p = p0 + ((int64_t)t * LANES + lane) * V;
            full[t] = p >= j0 && p + V <= j1;
            if (full[t]) ld.vec(p, v[t]);
            else {
                for (int k = 0; k < V; ++k)
                    if (p + k >= j0 && p + k < j1) v[t][k] = ld.one(p + k);
            }
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int t = 0; t < TILES_AHEAD; ++t) {
            const int64_t p = p0 + ((int64_t)t * LANES + lane) * V;
            for (int k = 0; k < V; ++k) {
                if (full[t] || (p + k >= j0 && p + k < j1)) {
                    acc = Op::combine(acc, Op::term(v[t][k], p + k, prm), prm);
                    if (chain) ++*chain;
                }
            }
        }
    }
    return acc;
}

// ---- a lane of the strided route: elements j0 .. j1-1 of the line at m, `inc` elements apart
template <typename Op, typename T>
REDUCE_HD typename Op::Acc strided_walk(const T* m, int64_t inc, int64_t j0, int64_t j1, const Params& prm) {
    constexpr int AHEAD = 8;
    typename Op::Acc acc = Op::identity();
    for (int64_t j = j0; j < j1; j += AHEAD) {
        T cur[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int u = 0; u < AHEAD; ++u)
            if (j + u < j1) cur[u] = m[(j + u) * inc];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int u = 0; u < AHEAD; ++u)
            if (j + u < j1) acc = Op::combine(acc, Op::term(cur[u], j + u, prm), prm);
    }
    return acc;
}

// ---- a lane of the finish: partials lane, lane + 64, .. of a line's S
template <typename Op>
REDUCE_HD typename Op::Acc finish_walk(const typename Op::Acc* rec, int64_t S, int lane, const Params& prm) {
    typename Op::Acc acc = Op::identity();
    for (int64_t s = lane; s < S; s += LANES) acc = Op::combine(acc, rec[s], prm);
    return acc;
}

// ---- the fold of 64 accumulators as lane 0 sees it (the device does it with lane exchanges: lane l < off takes lane l + off)
template <typename Op> inline typename Op::Acc fold64(typename Op::Acc* a, const Params& prm) {
    for (int off = LANES / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) a[l] = Op::combine(a[l], a[l + off], prm);
    return a[0];
}

// ---- host emulation of a whole plan: `phase` = (address of element 0 / element size) mod V as the device would see it
template <typename Op, typename T>
inline void emulate(const T* in, void* out, const Geom& g, const Params& prm, int64_t phase, typename Op::Acc* rec, int64_t* depth_reached) {
    using Acc = typename Op::Acc;
    constexpr int V = 16 / (int)sizeof(T);
    int64_t deepest = 0;
    for (int64_t line = 0; line < g.lines; ++line) {
        for (int64_t s = 0; s < g.S; ++s) {
            const int64_t j0 = s * g.seglen, j1 = j0 + g.seglen < g.len ? j0 + g.seglen : g.len;
            Acc acc;
            if (g.route == ROUTE_CONTIGUOUS) {
                const T* m = in + line * g.len;
                const int64_t a = (phase + line * g.len + j0) % V;
                Acc lanes[LANES];
                for (int l = 0; l < LANES; ++l) {
                    int64_t chain = 0;
                    lanes[l] = lane_walk<Op, T>(HostLoad<T>{m}, j0, j1, a, l, prm, &chain);
                    if (chain + 6 > deepest) deepest = chain + 6;
                }
                acc = fold64<Op>(lanes, prm);
            } else {
                const int64_t i = line % g.inner, o = line / g.inner;
                acc = strided_walk<Op, T>(in + i + g.inner * g.len * o, g.inner, j0, j1, prm);
                if (j1 - j0 > deepest) deepest = j1 - j0;
            }
            if (g.S > 1) rec[line * g.S + s] = acc;
            else Op::store(out, line, acc);
        }
        if (g.S > 1) {
            Acc lanes[LANES];
            for (int l = 0; l < LANES; ++l) lanes[l] = finish_walk<Op>(rec + line * g.S, g.S, l, prm);
            Op::store(out, line, fold64<Op>(lanes, prm));
        }
    }
    if (depth_reached) *depth_reached = deepest + (g.S > 1 ? (g.S + LANES - 1) / LANES + 6 : 0);
}

}  // namespace reduceop
}  // namespace mdsp
