// The thread mappings of the deterministic reductions, for any operator written for the templates of reduce_op.h (reduce.hip: the operators of
// util.jl; estimation.hip: those of est_op.h).  Device translation units only.
//
// The array is (inner, len, outer), element (i, j, o) at i + inner (j + len o), reduced along j.
//   contiguous route (inner == 1): a wavefront per (line, segment), four per workgroup, nothing shared between them.  Tiles of 64 lanes x 16 bytes sit on
//       16-byte boundaries of the address whatever the alignment of the array; the ragged first and last vectors are loaded element by element, nothing
//       outside [j0, j1) is touched.  The 64 accumulators are folded with lane exchanges.
//   strided route (inner > 1): a lane per (i, o, segment) walking j; neighbouring lanes hold neighbouring i, so a wavefront reads contiguous runs.
// S == 1 is one launch that writes the results.  S > 1 is two launches on the caller's stream: the first stores one partial per (line, segment) into
// the workspace, the finish (a wavefront per line) adds them in a fixed order.  No atomics, no flags: nothing waits for another workgroup.
#pragma once

#include <algorithm>

#include "common.h"
#include "reduce_op.h"

namespace mdsp {
namespace reduceop {

template <typename T> struct DevLoad {
    const T* m;
    __device__ __forceinline__ void vec(int64_t p, T* v) const {
        const uint4 w = *reinterpret_cast<const uint4*>(m + p);
        __builtin_memcpy(v, &w, 16);
    }
    __device__ __forceinline__ T one(int64_t e) const { return m[e]; }
};

__device__ __forceinline__ int64_t shfl_down_i64(int64_t v, int off) { return (int64_t)__shfl_down((long long)v, off, 64); }
__device__ __forceinline__ Sum1 shfl_down_acc(Sum1 a, int off) { return Sum1{__shfl_down(a.s, off, 64)}; }
__device__ __forceinline__ Sum2 shfl_down_acc(Sum2 a, int off) { return Sum2{__shfl_down(a.num, off, 64), __shfl_down(a.den, off, 64)}; }
__device__ __forceinline__ Arg shfl_down_acc(Arg a, int off) { return Arg{__shfl_down(a.a, off, 64), shfl_down_i64(a.idx, off), shfl_down_i64(a.nan, off)}; }

// fold64 of reduce_op.h: lane l takes lane l + off; lane 0 ends with the result (the lanes above `off` compute values nobody uses).  Every lane of the
// wavefront must be here.
template <typename Op> __device__ __forceinline__ typename Op::Acc wave_fold(typename Op::Acc a, const Params& prm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = Op::combine(a, shfl_down_acc(a, off), prm);
    return a;
}

template <typename Op, typename T>
__global__ __launch_bounds__(256) void reduce_contiguous_kernel(const T* in, int64_t len, int64_t S, int64_t seglen, int64_t nunits, Params prm,
                                                                typename Op::Acc* rec, void* out) {
    constexpr int V = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < nunits; u += nwaves) {   // wave-uniform
        const int64_t line = u / S, s = u - line * S;
        const int64_t j0 = s * seglen, j1 = j0 + seglen < len ? j0 + seglen : len;
        const T* m = in + line * len;
        const int64_t a = (int64_t)((reinterpret_cast<uintptr_t>(m + j0) / sizeof(T)) % V);
        const typename Op::Acc acc = wave_fold<Op>(lane_walk<Op, T>(DevLoad<T>{m}, j0, j1, a, lane, prm), prm);
        if (lane == 0) {
            if (rec) rec[u] = acc;
            else Op::store(out, u, acc);
        }
    }
}

template <typename Op, typename T>
__global__ __launch_bounds__(256) void reduce_strided_kernel(const T* in, int64_t inner, int64_t len, int64_t outer, int64_t S, int64_t seglen,
                                                             int64_t nthreads, Params prm, typename Op::Acc* rec, void* out) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nthreads; g += step) {
        const int64_t i = g % inner, r = g / inner, o = r % outer, s = r / outer;
        const int64_t j0 = s * seglen, j1 = j0 + seglen < len ? j0 + seglen : len;
        const typename Op::Acc acc = strided_walk<Op, T>(in + i + inner * len * o, inner, j0, j1, prm);
        const int64_t line = i + inner * o;
        if (rec) rec[line * S + s] = acc;
        else Op::store(out, line, acc);
    }
}

template <typename Op>
__global__ __launch_bounds__(256) void reduce_finish_kernel(const typename Op::Acc* rec, int64_t lines, int64_t S, Params prm, void* out) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); line < lines; line += nwaves) {   // wave-uniform
        const typename Op::Acc acc = wave_fold<Op>(finish_walk<Op>(rec + line * S, S, lane, prm), prm);
        if (lane == 0) Op::store(out, line, acc);
    }
}

constexpr int64_t MAX_GRID = 1 << 20;   // workgroups per launch; the kernels stride over what is left

// the launches of one exec; ws: lines x S partials (S > 1)
template <typename Op, typename T> int launch_reduce(const Geom& g, const Params& prm, const void* in_dev, void* ws, void* out_dev, hipStream_t st) {
    using Acc = typename Op::Acc;
    const T* in = static_cast<const T*>(in_dev);
    Acc* rec = g.S > 1 ? static_cast<Acc*>(ws) : nullptr;
    const int64_t units = g.lines * g.S;
    const dim3 block(256);
    if (g.route == ROUTE_CONTIGUOUS) {
        const dim3 grid((unsigned)std::min(cdiv(units, 4), MAX_GRID));
        hipLaunchKernelGGL((reduce_contiguous_kernel<Op, T>), grid, block, 0, st, in, g.len, g.S, g.seglen, units, prm, rec, out_dev);
    } else {
        const dim3 grid((unsigned)std::min(cdiv(units, 256), MAX_GRID));
        hipLaunchKernelGGL((reduce_strided_kernel<Op, T>), grid, block, 0, st, in, g.inner, g.len, g.outer, g.S, g.seglen, units, prm, rec, out_dev);
    }
    MDSP_LAUNCH_CHECK();
    if (g.S > 1) {
        const dim3 grid((unsigned)std::min(cdiv(g.lines, 4), MAX_GRID));
        hipLaunchKernelGGL((reduce_finish_kernel<Op>), grid, block, 0, st, static_cast<const Acc*>(rec), g.lines, g.S, prm, out_dev);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

}  // namespace reduceop
}  // namespace mdsp
