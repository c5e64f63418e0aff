// Device arithmetic shared by the FIR kernel families (fir.hip, fir_reg.hip, fir_creg.hip, fir_arb.hip, tdfir.hip): conversion to the accumulate type,
// the multiply-add chain's steps for real and complex taps, and the MDSP_NO_LSO kernel attribute (also fir_mm.hip, fir_dec.hip).  Internal to the library.
#pragma once

#include "fft_lds.h"

// The SI load / store optimizer per KERNEL (round 5 prep; round 4 switched it off for the whole FIR unit): merged ds_read2_b64 run at half rate and cost
// FIRArbitrary 8 %, 160//441 Float32 7 %, but the matrix-core kernel's fetched-tap and padded-run forms LOSE 6 - 13 % without the pass
// (profiles/r04_fir_lso_ab.json).  A function attribute decides it, and a body inlined into a kernel takes the kernel's setting.
// Device pass only: the host pass has no such target feature and would warn at every use.
#if defined(__HIP_DEVICE_COMPILE__)
#define MDSP_NO_LSO __attribute__((target("no-load-store-opt")))
#else
#define MDSP_NO_LSO
#endif

namespace mdsp {
namespace firop {

using fft::cx;

template <typename R> __device__ __forceinline__ R to_acc(float v, R*) { return (R)v; }
template <typename R> __device__ __forceinline__ R to_acc(double v, R*) { return (R)v; }
template <typename R> __device__ __forceinline__ cx<R> to_acc(cx<float> v, cx<R>*) { return {(R)v.x, (R)v.y}; }
template <typename R> __device__ __forceinline__ cx<R> to_acc(cx<double> v, cx<R>*) { return {(R)v.x, (R)v.y}; }
template <typename R> __device__ __forceinline__ void fma_acc(R& acc, R h, R x) { acc = fma(x, h, acc); }
template <typename R> __device__ __forceinline__ void fma_acc(cx<R>& acc, R h, cx<R> x) {
    acc.x = fma(x.x, h, acc.x);
    acc.y = fma(x.y, h, acc.y);
}
template <typename R> __device__ __forceinline__ R mul_first(R h, R x) { return h * x; }
template <typename R> __device__ __forceinline__ cx<R> mul_first(R h, cx<R> x) { return {h * x.x, h * x.y}; }
// complex taps (generic unsafe_dot, util.jl:225-283: the plain complex product, no conjugate): h x = h.re (x.re, x.im) + h.im (-x.im, x.re), in that order
template <typename R> __device__ __forceinline__ void fma_acc(cx<R>& acc, cx<R> h, R x) {
    acc.x = fma(x, h.x, acc.x);
    acc.y = fma(x, h.y, acc.y);
}
template <typename R> __device__ __forceinline__ void fma_acc(cx<R>& acc, cx<R> h, cx<R> x) {
    acc.x = fma(h.x, x.x, acc.x);
    acc.y = fma(h.x, x.y, acc.y);
    acc.x = fma(h.y, -x.y, acc.x);
    acc.y = fma(h.y, x.x, acc.y);
}
template <typename R> __device__ __forceinline__ cx<R> mul_first(cx<R> h, R x) { return {h.x * x, h.y * x}; }
template <typename R> __device__ __forceinline__ cx<R> mul_first(cx<R> h, cx<R> x) { return {fma(h.y, -x.y, h.x * x.x), fma(h.y, x.x, h.x * x.y)}; }

// 2 a - b  (extrapolate_signal!)
template <typename R> __device__ __forceinline__ R sub2(R a, R b) { return (R)2 * a - b; }
template <typename R> __device__ __forceinline__ cx<R> sub2(cx<R> a, cx<R> b) { return {(R)2 * a.x - b.x, (R)2 * a.y - b.y}; }
// muladd(yUpper, alpha::Float64, yLower) evaluated in Float64 and rounded once to the buffer's element type
__device__ __forceinline__ float arb_combine(float up, double al, float lo) { return (float)fma((double)up, al, (double)lo); }
__device__ __forceinline__ double arb_combine(double up, double al, double lo) { return fma(up, al, lo); }
__device__ __forceinline__ cx<float> arb_combine(cx<float> up, double al, cx<float> lo) {
    return {(float)fma((double)up.x, al, (double)lo.x), (float)fma((double)up.y, al, (double)lo.y)};
}
__device__ __forceinline__ cx<double> arb_combine(cx<double> up, double al, cx<double> lo) { return {fma(up.x, al, lo.x), fma(up.y, al, lo.y)}; }

}  // namespace firop
}  // namespace mdsp
