// Deterministic reductions along one dimension on the device (rms, rmsfft, meanfreq, finddelay of src/util.jl).  The operators, the geometry and the
// walk of a lane are reduce_op.h (shared with the host emulation, which therefore adds in the same order); here are the thread mappings and the C ABI.
//
// The array is (inner, len, outer), element (i, j, o) at i + inner (j + len o), reduced along j.
//   contiguous route (inner == 1): a wavefront per (line, segment), four per workgroup, nothing shared between them.  Tiles of 64 lanes x 16 bytes sit on
//       16-byte boundaries of the address whatever the alignment of the array; the ragged first and last vectors are loaded element by element, nothing
//       outside [j0, j1) is touched.  The 64 accumulators are folded with lane exchanges.
//   strided route (inner > 1): a lane per (i, o, segment) walking j; neighbouring lanes hold neighbouring i, so a wavefront reads contiguous runs.
// S == 1 is one launch that writes the results.  S > 1 is two launches on the caller's stream: the first stores one partial per (line, segment) into
// the plan's workspace, the finish (a wavefront per line) adds them in a fixed order.  No atomics, no flags: nothing waits for another workgroup.
#include <algorithm>
#include <vector>

#include "common.h"
#include "reduce_op.h"

using namespace mdsp;
using namespace mdsp::reduceop;

namespace {

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

bool op_takes(int op, int dtype) {
    if (op == OP_SUMABS2) return dtype_valid(dtype);
    if (op == OP_SUMABS2_W) return dtype_is_complex(dtype);
    if (op == OP_ABSARGMAX) return dtype == MDSP_F32 || dtype == MDSP_F64;
    return false;
}

int check_shape(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, bool* empty) {
    if (inner < 0 || len < 0 || outer < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: negative size (%lld, %lld, %lld)", (long long)inner, (long long)len, (long long)outer);
    if (op < OP_SUMABS2 || op > OP_ABSARGMAX) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: unknown operator %d", op);
    if (!op_takes(op, dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: operator %d does not take dtype %d", op, dtype);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    *empty = inner == 0 || outer == 0;
    int64_t n = 0;
    if (!*empty && (__builtin_mul_overflow(inner, std::max<int64_t>(len, 1), &n) || __builtin_mul_overflow(n, outer, &n) || n > (INT64_MAX >> 6)))
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: array too large");
    return MDSP_OK;
}

Geom geometry(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments) {
    return make_geometry(inner, len, outer, op, (int64_t)dtype_size(dtype), dtype_is_complex(dtype), segments);
}

}  // namespace

struct mdsp_reduce_plan_s {
    Geom g;
    int op = OP_SUMABS2, dtype = MDSP_F32;
    Params prm{0.0, 0};
    bool empty = false;
    DevBuf ws;   // S > 1: lines x S partials
};

namespace {

template <typename Op, typename T> int reduce_exec(mdsp_reduce_plan pl, const void* in_dev, void* out_dev, hipStream_t st) {
    using Acc = typename Op::Acc;
    const Geom& g = pl->g;
    const T* in = static_cast<const T*>(in_dev);
    Acc* rec = g.S > 1 ? pl->ws.as<Acc>() : nullptr;
    const int64_t units = g.lines * g.S;
    const dim3 block(256);
    if (g.route == ROUTE_CONTIGUOUS) {
        const dim3 grid((unsigned)std::min(cdiv(units, 4), MAX_GRID));
        hipLaunchKernelGGL((reduce_contiguous_kernel<Op, T>), grid, block, 0, st, in, g.len, g.S, g.seglen, units, pl->prm, rec, out_dev);
    } else {
        const dim3 grid((unsigned)std::min(cdiv(units, 256), MAX_GRID));
        hipLaunchKernelGGL((reduce_strided_kernel<Op, T>), grid, block, 0, st, in, g.inner, g.len, g.outer, g.S, g.seglen, units, pl->prm, rec, out_dev);
    }
    MDSP_LAUNCH_CHECK();
    if (g.S > 1) {
        const dim3 grid((unsigned)std::min(cdiv(g.lines, 4), MAX_GRID));
        hipLaunchKernelGGL((reduce_finish_kernel<Op>), grid, block, 0, st, static_cast<const Acc*>(rec), g.lines, g.S, pl->prm, out_dev);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

template <typename Op, typename T>
void emulate_as(const void* in, void* out, const Geom& g, const Params& prm, int64_t phase, int64_t* depth_reached) {
    std::vector<typename Op::Acc> rec((size_t)(g.S > 1 ? g.lines * g.S : 1));
    emulate<Op, T>(static_cast<const T*>(in), out, g, prm, phase, rec.data(), depth_reached);
}

// F(Op, T) for the (operator, element type) pairs of op_takes
#define MDSP_REDUCE_DISPATCH(op, dtype, F)                                                  \
    switch ((op) * 4 + (dtype)) {                                                           \
        case OP_SUMABS2 * 4 + MDSP_F32: F(OpSumAbs2, float); break;                          \
        case OP_SUMABS2 * 4 + MDSP_F64: F(OpSumAbs2, double); break;                         \
        case OP_SUMABS2 * 4 + MDSP_C32: F(OpSumAbs2, c32); break;                            \
        case OP_SUMABS2 * 4 + MDSP_C64: F(OpSumAbs2, c64); break;                            \
        case OP_SUMABS2_W * 4 + MDSP_C32: F(OpSumAbs2W, c32); break;                         \
        case OP_SUMABS2_W * 4 + MDSP_C64: F(OpSumAbs2W, c64); break;                         \
        case OP_ABSARGMAX * 4 + MDSP_F32: F(OpAbsArgmax, float); break;                      \
        default: F(OpAbsArgmax, double); break;                                             \
    }

}  // namespace

extern "C" {

int mdsp_reduce_geometry_for(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, int* route, int64_t* nsegments,
                             int64_t* seglen, int64_t* depth, int64_t* workspace_bytes) {
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, op, dtype, segments, &empty));
    const Geom g = geometry(inner, len, outer, op, dtype, segments);
    if (route) *route = g.route;
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (depth) *depth = g.depth;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_reduce_plan_create(mdsp_reduce_plan* plan, int64_t inner, int64_t len, int64_t outer, int op, int dtype, double step, int64_t centre,
                            int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, op, dtype, segments, &empty));
    if (op == OP_ABSARGMAX && centre < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: centre must be >= 0, got %lld", (long long)centre);
    auto pl = new mdsp_reduce_plan_s();
    pl->g = geometry(inner, len, outer, op, dtype, segments);
    pl->op = op;
    pl->dtype = dtype;
    pl->prm = Params{step, centre};
    pl->empty = empty;
    if (pl->g.workspace > 0) {
        const int st = pl->ws.reserve((size_t)pl->g.workspace);
        if (st != MDSP_OK) {
            delete pl;
            return st;
        }
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_reduce_plan_destroy(mdsp_reduce_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_reduce_plan_info(mdsp_reduce_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* depth, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (route) *route = plan->g.route;
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (depth) *depth = plan->g.depth;
    if (workspace_bytes) *workspace_bytes = (int64_t)plan->ws.bytes;
    return MDSP_OK;
}

int mdsp_reduce_exec(mdsp_reduce_plan plan, const void* in_dev, void* out_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (plan->empty) return MDSP_OK;
    if (!out_dev || (!in_dev && plan->g.len > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(in_dev) % dtype_size(plan->dtype) || reinterpret_cast<uintptr_t>(out_dev) % 8)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: the array must be aligned to its element size, the result to 8 bytes");
    hipStream_t st = as_stream(stream);
#define MDSP_REDUCE_EXEC(Op, T) return reduce_exec<Op, T>(plan, in_dev, out_dev, st)
    MDSP_REDUCE_DISPATCH(plan->op, plan->dtype, MDSP_REDUCE_EXEC)
#undef MDSP_REDUCE_EXEC
    return MDSP_OK;
}

int mdsp_reduce_emulate(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int op, int dtype, double step, int64_t centre,
                        int64_t segments, int64_t phase, int64_t* depth_reached) {
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, op, dtype, segments, &empty));
    if (phase < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "reduce: phase must be >= 0");
    if (depth_reached) *depth_reached = 0;
    if (empty) return MDSP_OK;
    if (!out_host || (!in_host && len > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const Geom g = geometry(inner, len, outer, op, dtype, segments);
    const Params prm{step, centre};
#define MDSP_REDUCE_EMULATE(Op, T) emulate_as<Op, T>(in_host, out_host, g, prm, phase, depth_reached)
    MDSP_REDUCE_DISPATCH(op, dtype, MDSP_REDUCE_EMULATE)
#undef MDSP_REDUCE_EMULATE
    return MDSP_OK;
}

}  // extern "C"
