// unwrap along one dimension (src/unwrap.jl:17-34) as a scan.
//
//     y[0] = m[0];   y[i] = m[i] - round((m[i] - y[i-1]) / range) * range                    (accumulate!(unwrap_kernel(range), y, m; dims))
//
// With q_i = (m[i] - m[i-1]) / range, d_i = rint(q_i) and K_i = d_1 + ... + d_i (integers) the result is y[i] = m[i] - T(K_i) * range: an integer
// prefix sum, associative, so a line may be cut anywhere.  The arithmetic is the reference's, in T: one IEEE subtraction and one division for q,
// rint (ties to even, Julia's round), one product and one subtraction for y.  The library is compiled with -ffp-contract=on, which would turn
// m - T(K) * range into one fused multiply-add and change the low bit; every operation below is therefore a function of its own (the device
// forms __fmul_rn / __fsub_rn / __fdiv_rn and their __d*_rn twins; on the host a function per operation, contraction never crosses a call).
//
// Non-finite samples follow the recurrence through a small absorbing state beside K: a non-finite m[i], i >= 1, makes the rest of the line NaN;
// m[0] = NaN makes the whole line NaN; m[0] = +-Inf followed by finite samples gives a line of +-Inf.
//
// A line of `len` samples is cut into S segments of `seglen` (the last one ragged).  Three steps, each a launch of its own on the device:
//   1. reduce  : per segment the sum of d and the state, INCLUDING the increment at the segment's first sample (which reads the last sample of the
//                segment before it) -- kept apart as (bK, bst) as well
//   2. carries : exclusive scan of the records of a line; the carry of segment s is (everything before s) (+) (its own boundary increment)
//   3. apply   : the carry is K and the state AT the segment's first sample; the segment walks on from its own samples and never reads the
//                sample in front of it (in place, that sample may already hold the result of another segment).
// Everything here is shared by the kernels (unwrap.hip) and the host emulation (mdsp_unwrap_emulate_host), which runs the same text.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define UNWRAP_HD __host__ __device__ inline
#else
#define UNWRAP_HD inline
#endif

namespace mdsp {
namespace unwrapscan {

enum : int { ST_FIN = 0, ST_PINF = 1, ST_NINF = 2, ST_NAN = 3 };
enum : int { ROUTE_CONTIGUOUS = 0, ROUTE_STRIDED = 1 };

// K is summed modulo 2^64 (unsigned: no overflow to define away); it is an integer of the documented range (|K| < 2^24 / 2^53) reinterpreted.
struct Acc {
    uint64_t K;
    int st;
};
// what step 1 leaves per segment, and (K, st overwritten by step 2) what step 3 starts from
struct Rec {
    uint64_t K;    // step 1: sum of d over the segment, boundary increment included; step 2: the carry
    uint64_t bK;   // the boundary increment alone (first segment of a line: 0, with the start state in bst)
    int32_t st;    // as K
    int32_t bst;   // as bK
};

// ---- one rounding per operation
UNWRAP_HD float sub_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
UNWRAP_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
UNWRAP_HD float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
UNWRAP_HD double sub_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
UNWRAP_HD double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
UNWRAP_HD double div_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
UNWRAP_HD float rint_t(float q) { return rintf(q); }
UNWRAP_HD double rint_t(double q) { return rint(q); }

template <typename T> UNWRAP_HD bool finite_t(T v) { return sub_rn(v, v) == (T)0; }   // false for +-Inf and NaN

// ---- the scan operator: `a` earlier on the line than `b`.  FIN is the identity; a start state (+-Inf, NaN at sample 0) has nothing before it;
// every other event is NaN, and NaN after anything non-finite stays NaN.
UNWRAP_HD int combine_state(int a, int b) { return b == ST_FIN ? a : (a == ST_FIN ? b : ST_NAN); }
UNWRAP_HD Acc combine(Acc a, Acc b) { return Acc{a.K + b.K, combine_state(a.st, b.st)}; }

// sample 0 of a line
template <typename T> UNWRAP_HD Acc start_event(T m) {
    return Acc{0, finite_t(m) ? ST_FIN : (m != m ? ST_NAN : (m > (T)0 ? ST_PINF : ST_NINF))};
}
// sample i >= 1 with its left neighbour: (d_i, event).  A non-finite sample is the NaN event; behind a non-finite neighbour the state is
// already absorbing and d does not matter.  An increment that does not fit (|q| >= 2^62: far beyond the documented range) is the NaN event too:
// the conversion to an integer stays defined.
template <typename T> UNWRAP_HD Acc step_event(T prev, T cur, T range) {
    if (!finite_t(cur)) return Acc{0, ST_NAN};
    if (!finite_t(prev)) return Acc{0, ST_FIN};
    const T d = rint_t(div_rn(sub_rn(cur, prev), range));
    if (!(d > (T)-4.6e18 && d < (T)4.6e18)) return Acc{0, ST_NAN};
    return Acc{(uint64_t)(int64_t)d, ST_FIN};
}
// y[i] from m[i] and the inclusive scan at i
template <typename T> UNWRAP_HD T finish(T m, Acc a, T range) {
    if (a.st == ST_FIN) return sub_rn(m, mul_rn((T)(int64_t)a.K, range));
    if (a.st == ST_PINF) return (T)INFINITY;
    if (a.st == ST_NINF) return -(T)INFINITY;
    return (T)NAN;
}

// ---- geometry: pure host arithmetic.  The cut does not depend on the device the plan lands on (256 compute units are assumed), so that
// mdsp_unwrap_geometry_for needs none and a result does not depend on the machine.
struct Geom {
    int route = ROUTE_CONTIGUOUS;
    int64_t inner = 0, len = 0, outer = 0, lines = 0, S = 1, seglen = 0, workspace = 0;
};
constexpr int64_t WAVES_TARGET = 256 * 32;             // contiguous route: a wavefront per (line, segment), 32 resident per compute unit
constexpr int64_t LANES_TARGET = WAVES_TARGET * 64;    // strided route: a lane per (inner index, outer index, segment)
constexpr int64_t MINSEG_CONTIGUOUS = 4096, MINSEG_STRIDED = 256;   // shortest segments of an automatic cut (a forced one goes down to 1)

inline Geom make_geometry(int64_t inner, int64_t len, int64_t outer, int64_t segments) {
    Geom g;
    g.route = inner == 1 ? ROUTE_CONTIGUOUS : ROUTE_STRIDED;
    g.inner = inner;
    g.len = len;
    g.outer = outer;
    g.lines = inner * outer;
    g.seglen = len;
    if (g.lines == 0 || len == 0) return g;
    int64_t want = 1;
    if (len <= 2) want = 1;
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
    g.S = (len + g.seglen - 1) / g.seglen;   // no empty segment: S <= want, equal wherever want divides len nearly evenly
    g.workspace = g.S > 1 ? g.lines * g.S * (int64_t)sizeof(Rec) : 0;
    return g;
}

// ---- the per-segment walk.  Samples j0 .. j1-1 of the line at `m` (stride `inc` elements).  MODE 0: the whole line in one pass (j0 = 0);
// MODE 1: the segment's record; MODE 2: apply from the carry.  `y` may be `m`: sample j is read before y[j] is written and travels in `prev`.
template <int MODE, typename T> UNWRAP_HD void walk_segment(const T* m, T* y, int64_t inc, int64_t j0, int64_t j1, T range, Rec* rec) {
    Acc a{0, ST_FIN}, b{0, ST_FIN};
    T prev = m[j0 * inc];
    if (MODE == 2) a = Acc{rec->K, rec->st};                              // K and the state AT sample j0: m[j0 - 1] is not read
    else if (j0 == 0) a = b = start_event(prev);                         // the "boundary" of a line's first segment is its start state
    else a = b = step_event(m[(j0 - 1) * inc], prev, range);             // MODE 1 only: j0 > 0 means S > 1
    if (MODE != 1) y[j0 * inc] = finish(prev, a, range);
    // WALK_AHEAD samples are read before the first of them is written: y is m or does not overlap it, so a store to y[j] can only hit the
    // sample j already in hand -- said here because the compiler cannot know it and would otherwise keep one load in flight per lane.
    constexpr int WALK_AHEAD = 8;
    for (int64_t j = j0 + 1; j < j1; j += WALK_AHEAD) {
        T cur[WALK_AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int u = 0; u < WALK_AHEAD; ++u) cur[u] = j + u < j1 ? m[(j + u) * inc] : (T)0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int u = 0; u < WALK_AHEAD; ++u) {
            if (j + u < j1) {
                a = combine(a, step_event(prev, cur[u], range));
                if (MODE != 1) y[(j + u) * inc] = finish(cur[u], a, range);
                prev = cur[u];
            }
        }
    }
    if (MODE == 1) *rec = Rec{a.K, b.K, a.st, b.st};
}

// step 2 for one line, serially (the host emulation; the device scans 64 records at a time with the same operator)
inline void scan_carries(Rec* rec, int64_t S) {
    Acc run{0, ST_FIN};
    for (int64_t s = 0; s < S; ++s) {
        const Acc total{rec[s].K, rec[s].st}, carry = combine(run, Acc{rec[s].bK, rec[s].bst});
        rec[s].K = carry.K;
        rec[s].st = carry.st;
        run = combine(run, total);
    }
}

}  // namespace unwrapscan
}  // namespace mdsp
