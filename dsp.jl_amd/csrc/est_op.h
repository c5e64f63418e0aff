// The reductions of the frequency estimators (src/estimation.jl:93-115, :164, :196) as operators for the templates of reduce_op.h -- lane_walk,
// strided_walk, finish_walk, fold64, emulate and the cut of make_geometry -- which this header uses as they are: the order of additions is the one
// reduce_op.h writes down.  The operators of mdsp_reduce_* keep their numbers; these two have an ABI of their own (mdsp_est_reduce_*):
//
//   SUM          the Float64 sum of the elements of a line, every element converted exactly to Float64; a complex line gives two sums (re, im).
//                mean(x) of quinn is SUM / N.
//   ABS2ARGMAX   complex bins X_k: the index of the largest abs2_f64(X_k) (the Float64 |X|^2 of reduce_op.h); at equal value the smaller index,
//                findmax's first maximum (estimation.jl:96; abs and abs2 order the bins alike but for roundings, and abs2 needs no square root).
//                The rule is a total order, so the operator is associative and commutative and the result does not depend on the cut.  A bin whose
//                abs2 is NaN does not compete and raises the flag.
//
// and the gather of the peak's neighbours (estimation.jl:98-107), one record of 64 bytes.
// Everything here is shared by the kernels (estimation.hip) and the host emulations, which run the same text.
#pragma once

#include "reduce_op.h"

namespace mdsp {
namespace estop {

using reduceop::Arg;
using reduceop::c32;
using reduceop::c64;
using reduceop::Params;
using reduceop::Sum1;
using reduceop::Sum2;

enum : int { OP_SUM = 0, OP_ABS2ARGMAX = 1 };

struct OpSumReal {
    using Acc = Sum1;
    static constexpr int NOUT = 1;
    REDUCE_HD static Acc identity() { return Acc{0.0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t, const Params&) { return Acc{(double)x}; }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params&) { return Acc{reduceop::add_rn(a.s, b.s)}; }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) { static_cast<double*>(out)[line] = a.s; }
};
struct OpSumCplx {   // Sum2 as (re, im)
    using Acc = Sum2;
    static constexpr int NOUT = 2;
    REDUCE_HD static Acc identity() { return Acc{0.0, 0.0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t, const Params&) { return Acc{(double)x.re, (double)x.im}; }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params&) { return Acc{reduceop::add_rn(a.num, b.num), reduceop::add_rn(a.den, b.den)}; }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) {
        static_cast<double*>(out)[2 * line] = a.num;
        static_cast<double*>(out)[2 * line + 1] = a.den;
    }
};
struct OpAbs2Argmax {   // Arg.a: abs2 of the candidate; -1: none yet
    using Acc = Arg;
    static constexpr int NOUT = 2;
    REDUCE_HD static Acc identity() { return Acc{-1.0, -1, 0}; }
    template <typename T> REDUCE_HD static Acc term(T x, int64_t k, const Params&) {
        const double v = reduceop::abs2_f64(x);
        if (v != v) return Acc{-1.0, -1, 1};
        return Acc{v, k, 0};
    }
    REDUCE_HD static Acc combine(Acc a, Acc b, const Params&) {
        const bool takeb = b.a > a.a || (b.a == a.a && b.idx < a.idx);   // (an identity never wins: -1 < every abs2, and -1 == -1 keeps a)
        return Acc{takeb ? b.a : a.a, takeb ? b.idx : a.idx, a.nan | b.nan};
    }
    REDUCE_HD static void store(void* out, int64_t line, Acc a) {   // the record (index, flag): two ordinary 8-byte stores
        static_cast<int64_t*>(out)[2 * line] = a.idx;
        static_cast<int64_t*>(out)[2 * line + 1] = a.nan;
    }
};

inline int64_t acc_bytes(int op, bool is_complex) { return op == OP_ABS2ARGMAX ? (int64_t)sizeof(Arg) : is_complex ? (int64_t)sizeof(Sum2) : (int64_t)sizeof(Sum1); }

// the cut of reduce_op.h with this header's partials in the workspace (a complex SUM term is two conversions, no addition inside it)
inline reduceop::Geom make_geometry(int64_t inner, int64_t len, int64_t outer, int op, int64_t elem_bytes, bool is_complex, int64_t segments) {
    reduceop::Geom g = reduceop::make_geometry(inner, len, outer, reduceop::OP_SUMABS2, elem_bytes, op == OP_ABS2ARGMAX, segments);
    g.workspace = g.S > 1 ? g.lines * g.S * acc_bytes(op, is_complex) : 0;
    return g;
}

// ---- the peak record of jacobsen: eight 8-byte words
//   [0] index k of the peak, 0-based (Int64; -1: no bin competed)   [1] NaN flag (Int64)   [2..3] X[k-1]   [4..5] X[k]   [6..7] X[k+1]   (re, im in Float64)
// with the reference's wrap-around for a full transform of n bins (X[-1] = X[n-1], X[n] = X[0], estimation.jl:98-103) and the Hermitian mirror at the ends
// of a one-sided spectrum of n / 2 + 1 bins: X[-1] = conj(X[1]), and X[k+1] = conj(X[n-k-1]) where k + 1 is beyond the last bin (the Nyquist bin of an
// even n: conj(X[k-1]); the last bin of an odd n: conj(X[k])).  n >= 2, so every bin named exists.
constexpr int PEAK_WORDS = 8;

template <typename C> REDUCE_HD void peak_record(const C* bins, int64_t nbins, int64_t n, int onesided, const int64_t* argmax, void* out) {
    int64_t* oi = static_cast<int64_t*>(out);
    double* od = static_cast<double*>(out);
    const int64_t k = argmax[0];
    oi[0] = k;
    oi[1] = argmax[1];
    for (int i = 2; i < PEAK_WORDS; ++i) od[i] = 0.0;
    if (k < 0 || k >= nbins) return;
    int64_t im1 = k - 1, ip1 = k + 1;
    double sm1 = 1.0, sp1 = 1.0;   // the sign of the imaginary part: -1 for a mirrored bin
    if (onesided) {
        if (k == 0) { im1 = 1; sm1 = -1.0; }
        if (ip1 >= nbins) { ip1 = n - k - 1; sp1 = -1.0; }
    } else {
        if (k == 0) im1 = n - 1;
        if (ip1 >= n) ip1 = 0;
    }
    od[2] = (double)bins[im1].re;
    od[3] = sm1 * (double)bins[im1].im;
    od[4] = (double)bins[k].re;
    od[5] = (double)bins[k].im;
    od[6] = (double)bins[ip1].re;
    od[7] = sp1 * (double)bins[ip1].im;
}

}  // namespace estop
}  // namespace mdsp
