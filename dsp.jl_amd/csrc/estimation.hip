// jacobsen and quinn (src/estimation.jl:93-220) on the device.  The reductions' operators and the peak record are est_op.h, the arithmetic, the geometry
// and the powers of a pass quinn_scan.h (both shared with the host emulations); the reductions' thread mappings are reduce_kernels.h.  Here are the thread
// mapping of a pass, the iteration and the C ABI.
//
// A pass: a wavefront per segment, nothing shared between wavefronts.  A tile of 64 x RUN samples is loaded with consecutive lanes on consecutive
// samples -- in the signal's own type -- and handed to the lanes run by run through LDS (rows of RUN + 1 elements: lane l reading run l meets no bank
// twice within the lanes served together); nothing is stored but the record.  alpha, the mean and the powers travel in the kernel arguments, the state
// and the sums live in registers.  S == 1 is one launch; S > 1 is four on the caller's stream -- end states, carries, sums, finish -- every dependence
// between workgroups a kernel boundary: no flags, no atomics, nothing waits, and a record depends on the call's arguments only.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "est_op.h"
#include "quinn_scan.h"
#include "reduce_kernels.h"

using namespace mdsp;
using namespace mdsp::quinnscan;
namespace rop = mdsp::reduceop;
namespace eop = mdsp::estop;

namespace {

// ------------------------------------------------------------------------------------------------ the reductions
bool est_op_takes(int op, int dtype) {
    if (op == eop::OP_SUM) return dtype_valid(dtype);
    if (op == eop::OP_ABS2ARGMAX) return dtype_is_complex(dtype);
    return false;
}

int est_check_shape(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, bool* empty) {
    if (inner < 0 || len < 0 || outer < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: negative size (%lld, %lld, %lld)", (long long)inner, (long long)len, (long long)outer);
    if (op < eop::OP_SUM || op > eop::OP_ABS2ARGMAX) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: unknown operator %d", op);
    if (!est_op_takes(op, dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: operator %d does not take dtype %d", op, dtype);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    *empty = inner == 0 || outer == 0;
    int64_t n = 0;
    if (!*empty && (__builtin_mul_overflow(inner, std::max<int64_t>(len, 1), &n) || __builtin_mul_overflow(n, outer, &n) || n > (INT64_MAX >> 6)))
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: array too large");
    return MDSP_OK;
}

rop::Geom est_geometry(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments) {
    return eop::make_geometry(inner, len, outer, op, (int64_t)dtype_size(dtype), dtype_is_complex(dtype), segments);
}

// F(Op, T) for the (operator, element type) pairs of est_op_takes
#define MDSP_EST_DISPATCH(op, dtype, F)                                  \
    switch ((op) * 4 + (dtype)) {                                        \
        case eop::OP_SUM * 4 + MDSP_F32: F(eop::OpSumReal, float); break;     \
        case eop::OP_SUM * 4 + MDSP_F64: F(eop::OpSumReal, double); break;    \
        case eop::OP_SUM * 4 + MDSP_C32: F(eop::OpSumCplx, rop::c32); break;  \
        case eop::OP_SUM * 4 + MDSP_C64: F(eop::OpSumCplx, rop::c64); break;  \
        case eop::OP_ABS2ARGMAX * 4 + MDSP_C32: F(eop::OpAbs2Argmax, rop::c32); break; \
        default: F(eop::OpAbs2Argmax, rop::c64); break;                  \
    }

int est_reduce_launch(const rop::Geom& g, int op, int dtype, const void* in_dev, void* ws, void* out_dev, hipStream_t st) {
    const rop::Params prm{0.0, 0};
#define MDSP_EST_EXEC(Op, T) return (rop::launch_reduce<Op, T>(g, prm, in_dev, ws, out_dev, st))
    MDSP_EST_DISPATCH(op, dtype, MDSP_EST_EXEC)
#undef MDSP_EST_EXEC
    return MDSP_OK;
}

template <typename Op, typename T> void est_emulate_as(const void* in, void* out, const rop::Geom& g, int64_t phase, int64_t* depth_reached) {
    std::vector<typename Op::Acc> rec((size_t)(g.S > 1 ? g.lines * g.S : 1));
    rop::emulate<Op, T>(static_cast<const T*>(in), out, g, rop::Params{0.0, 0}, phase, rec.data(), depth_reached);
}

template <typename C> __global__ void peak_gather_kernel(const C* bins, int64_t nbins, int64_t n, int onesided, const int64_t* argmax, void* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) eop::peak_record<C>(bins, nbins, n, onesided, argmax, out);
}

int peak_check(int64_t nbins, int64_t n, int onesided, int dtype, const void* bins, const void* argmax, const void* out) {
    if (!dtype_is_complex(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_peak: the bins are MDSP_C32 or MDSP_C64 (got dtype %d)", dtype);
    if (n < 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_peak: at least two samples are needed (got %lld)", (long long)n);
    if (nbins != (onesided ? n / 2 + 1 : n))
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_peak: %lld bins do not belong to a %s transform of %lld samples", (long long)nbins, onesided ? "one-sided" : "full", (long long)n);
    if (!bins || !argmax || !out) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_peak: NULL buffer");
    return MDSP_OK;
}

// ------------------------------------------------------------------------------------------------ the pass
enum : int { MODE_WHOLE = 0, MODE_REDUCE = 1, MODE_APPLY = 2 };

template <bool CPLX> struct Args {
    Pass<CPLX> ps;
    int64_t n, S, seglen;
    double* ws_state;   // S > 1: NSTATE doubles per segment
    double* ws_part;    // S > 1: NSUM doubles per segment
    double* out;        // the record
    int mode;
};

template <bool CPLX> __device__ __forceinline__ void wave_scan(const double* mats, int lane, double* v) {
#pragma unroll
    for (int d = 0; d < LEVELS; ++d) {
        double u[NSTATE];
#pragma unroll
        for (int i = 0; i < NSTATE; ++i) u[i] = __shfl_up(v[i], 1 << d, 64);
        if (lane >= (1 << d)) affine_add<CPLX>(mats + d * Form<CPLX>::NMAT, u, v);
    }
}

// WPB wavefronts per workgroup (two for ComplexF64: 64 rows of 17 sixteen-byte elements each)
template <typename T, bool CPLX, bool SUMS, int WPB> __global__ __launch_bounds__(64 * WPB) void quinn_pass_kernel(const Args<CPLX> a, const T* x) {
    constexpr int NS = Form<CPLX>::NSUM;
    __shared__ T lds_all[WPB][64 * (RUN + 1)];
    const int lane = threadIdx.x & 63;
    T* lds = lds_all[threadIdx.x >> 6];
    const int64_t nwaves = (int64_t)gridDim.x * WPB;
    for (int64_t unit = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); unit < a.S; unit += nwaves) {   // wave-uniform
        const int64_t j0 = unit * a.seglen, j1 = j0 + a.seglen < a.n ? j0 + a.seglen : a.n;
        double z[NSTATE], v[NSTATE], u[NSTATE], acc[NS];
        T xs[RUN];
#pragma unroll
        for (int i = 0; i < NSTATE; ++i) z[i] = a.mode == MODE_APPLY ? a.ws_state[unit * NSTATE + i] : 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = 0.0;
        for (int64_t t0 = j0; t0 < j1; t0 += TILE) {
            const int cnt = (int)(j1 - t0 < TILE ? j1 - t0 : TILE);
            __builtin_amdgcn_wave_barrier();   // the reads of the tile before are done (the DS operations of a wavefront execute in order)
#pragma unroll
            for (int t = 0; t < RUN; ++t) {
                const int i = t * 64 + lane;
                if (i < cnt) lds[i + i / RUN] = x[t0 + i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            int mine = cnt - lane * RUN;
            mine = mine < 0 ? 0 : mine > RUN ? RUN : mine;
#pragma unroll
            for (int t = 0; t < RUN; ++t)
                if (t < mine) xs[t] = lds[lane * (RUN + 1) + t];
#pragma unroll
            for (int i = 0; i < NSTATE; ++i) v[i] = lane == 0 ? z[i] : 0.0;
            walk_run<CPLX, false, T>(a.ps.p, a.ps.mu, xs, mine, t0 + lane * RUN, a.n, v, nullptr, nullptr);
            wave_scan<CPLX>(a.ps.tile, lane, v);
#pragma unroll
            for (int i = 0; i < NSTATE; ++i) {
                u[i] = __shfl_up(v[i], 1, 64);
                if (lane == 0) u[i] = z[i];
            }
            walk_run<CPLX, SUMS, T>(a.ps.p, a.ps.mu, xs, mine, t0 + lane * RUN, a.n, u, acc, a.out + 2);   // from its true start state every run is the serial recurrence
            const int last = (cnt - 1) / RUN;
#pragma unroll
            for (int i = 0; i < NSTATE; ++i) z[i] = __shfl(u[i], last, 64);
        }
        if (SUMS) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i] = add_rn(acc[i], __shfl_down(acc[i], off, 64));
            }
            if (lane == 0) {
                double* dst = a.S > 1 ? a.ws_part + unit * NS : a.out;
#pragma unroll
                for (int i = 0; i < NS; ++i) dst[i] = acc[i];
            }
        } else if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NSTATE; ++i) a.ws_state[unit * NSTATE + i] = z[i];
        }
    }
}

// step 2: one wavefront, 64 records at a time; the records become the states at the segments' first samples
template <bool CPLX> __global__ __launch_bounds__(64) void quinn_carry_kernel(const Args<CPLX> a) {
    const int lane = threadIdx.x & 63;
    double r[NSTATE] = {0.0, 0.0}, v[NSTATE];
    for (int64_t s0 = 0; s0 < a.S; s0 += 64) {
        const int64_t s = s0 + lane;
#pragma unroll
        for (int i = 0; i < NSTATE; ++i) v[i] = s < a.S ? a.ws_state[s * NSTATE + i] : 0.0;
        if (lane == 0) affine_add<CPLX>(a.ps.seg, r, v);
        wave_scan<CPLX>(a.ps.seg, lane, v);
#pragma unroll
        for (int i = 0; i < NSTATE; ++i) {
            double c = __shfl_up(v[i], 1, 64);
            if (lane == 0) c = r[i];
            if (s < a.S) a.ws_state[s * NSTATE + i] = c;
            r[i] = __shfl(v[i], 63, 64);
        }
    }
}

// step 4: one wavefront adds the partials (finish_walk, then the fold)
template <bool CPLX> __global__ __launch_bounds__(64) void quinn_finish_kernel(const Args<CPLX> a) {
    constexpr int NS = Form<CPLX>::NSUM;
    using Op = OpSums<NS>;
    const int lane = threadIdx.x & 63;
    typename Op::Acc acc = rop::finish_walk<Op>(reinterpret_cast<const typename Op::Acc*>(a.ws_part), a.S, lane, rop::Params{0.0, 0});
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < NS; ++i) acc.s[i] = add_rn(acc.s[i], __shfl_down(acc.s[i], off, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) a.out[i] = acc.s[i];
    }
}

constexpr int64_t MAX_PASS_GRID = 1 << 16;

// the powers of this iteration; p: alpha or omega
template <bool CPLX> int make_pass(const Geom& g, double param, const double* mean, Pass<CPLX>* ps) {
    if (CPLX) {
        ps->p[0] = std::cos(param);
        ps->p[1] = std::sin(param);
    } else {
        ps->p[0] = param;
        ps->p[1] = 0.0;
    }
    ps->mu[0] = mean[0];
    ps->mu[1] = CPLX ? mean[1] : 0.0;
    for (int i = 0; i < LEVELS * Form<CPLX>::NMAT; ++i) ps->seg[i] = 0.0;
    if (!std::isfinite(ps->p[0]) || !std::isfinite(ps->p[1]) || !power_ladder<CPLX>(ps->p, RUN, ps->tile) || (g.S > 1 && !power_ladder<CPLX>(ps->p, g.seglen, ps->seg)))
        MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "quinn: the powers of the recurrence's matrix are not finite in Float64 (the iterate %.17g left the unit circle): use DSP.jl's CPU path", param);
    return MDSP_OK;
}

template <typename T, bool CPLX, int WPB> int pass_launch(const Geom& g, const Pass<CPLX>& ps, const void* x_dev, double* ws, double* out_dev, hipStream_t st) {
    Args<CPLX> a{};
    a.ps = ps;
    a.n = g.n;
    a.S = g.S;
    a.seglen = g.seglen;
    a.ws_state = ws;
    a.ws_part = ws ? ws + g.S * NSTATE : nullptr;
    a.out = out_dev;
    const T* x = static_cast<const T*>(x_dev);
    const dim3 grid((unsigned)std::min(cdiv(g.S, WPB), MAX_PASS_GRID)), block(64 * WPB);
    if (g.S == 1) {
        a.mode = MODE_WHOLE;
        hipLaunchKernelGGL((quinn_pass_kernel<T, CPLX, true, WPB>), grid, block, 0, st, a, x);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    a.mode = MODE_REDUCE;
    hipLaunchKernelGGL((quinn_pass_kernel<T, CPLX, false, WPB>), grid, block, 0, st, a, x);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((quinn_carry_kernel<CPLX>), dim3(1), dim3(64), 0, st, a);
    MDSP_LAUNCH_CHECK();
    a.mode = MODE_APPLY;
    hipLaunchKernelGGL((quinn_pass_kernel<T, CPLX, true, WPB>), grid, block, 0, st, a, x);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((quinn_finish_kernel<CPLX>), dim3(1), dim3(64), 0, st, a);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

int quinn_check(int dtype, int64_t n, int64_t segments) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: bad dtype %d", dtype);
    if (n < 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: at least two samples are needed (got %lld)", (long long)n);
    if (n > (INT64_MAX >> 6)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: signal too long");
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    return MDSP_OK;
}

}  // namespace

struct mdsp_est_reduce_plan_s {
    rop::Geom g;
    int op = eop::OP_SUM, dtype = MDSP_F32;
    bool empty = false;
    DevBuf ws;   // S > 1: lines x S partials
};

struct mdsp_quinn_plan_s {
    Geom g;
    int dtype = MDSP_F32;
    rop::Geom gsum;          // the SUM reduction behind the mean
    std::mutex mu;
    DevBuf ws, sumws, rec;   // the plan touches the device at its first exec, not before; rec: 2 doubles of the sum, then the pass record
};

namespace {

int ensure_device(mdsp_quinn_plan pl) {
    std::lock_guard<std::mutex> lock(pl->mu);
    if (pl->g.workspace > 0) MDSP_TRY(pl->ws.reserve((size_t)pl->g.workspace));
    if (pl->gsum.workspace > 0) MDSP_TRY(pl->sumws.reserve((size_t)pl->gsum.workspace));
    return pl->rec.reserve(8 * 8);
}

int pass_exec(mdsp_quinn_plan pl, const void* x_dev, const double* mean, double param, double* out_dev, hipStream_t st) {
    const Geom& g = pl->g;
    double* ws = pl->ws.as<double>();
    if (g.cplx) {
        Pass<true> ps;
        MDSP_TRY(make_pass<true>(g, param, mean, &ps));
        return pl->dtype == MDSP_C32 ? pass_launch<rop::c32, true, 4>(g, ps, x_dev, ws, out_dev, st) : pass_launch<rop::c64, true, 2>(g, ps, x_dev, ws, out_dev, st);
    }
    Pass<false> ps;
    MDSP_TRY(make_pass<false>(g, param, mean, &ps));
    return pl->dtype == MDSP_F32 ? pass_launch<float, false, 4>(g, ps, x_dev, ws, out_dev, st) : pass_launch<double, false, 4>(g, ps, x_dev, ws, out_dev, st);
}

int exec_check(mdsp_quinn_plan plan, const void* x_dev) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (!x_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: NULL buffer");
    if (reinterpret_cast<uintptr_t>(x_dev) % dtype_size(plan->dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: the signal must be aligned to its element size");
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_est_reduce_geometry_for(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, int* route, int64_t* nsegments,
                                 int64_t* seglen, int64_t* depth, int64_t* workspace_bytes) {
    bool empty = false;
    MDSP_TRY(est_check_shape(inner, len, outer, op, dtype, segments, &empty));
    const rop::Geom g = est_geometry(inner, len, outer, op, dtype, segments);
    if (route) *route = g.route;
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (depth) *depth = g.depth;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_est_reduce_plan_create(mdsp_est_reduce_plan* plan, int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    bool empty = false;
    MDSP_TRY(est_check_shape(inner, len, outer, op, dtype, segments, &empty));
    auto pl = new mdsp_est_reduce_plan_s();
    pl->g = est_geometry(inner, len, outer, op, dtype, segments);
    pl->op = op;
    pl->dtype = dtype;
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

int mdsp_est_reduce_plan_destroy(mdsp_est_reduce_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_est_reduce_plan_info(mdsp_est_reduce_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* depth, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (route) *route = plan->g.route;
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (depth) *depth = plan->g.depth;
    if (workspace_bytes) *workspace_bytes = (int64_t)plan->ws.bytes;
    return MDSP_OK;
}

int mdsp_est_reduce_exec(mdsp_est_reduce_plan plan, const void* in_dev, void* out_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (plan->empty) return MDSP_OK;
    if (!out_dev || (!in_dev && plan->g.len > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(in_dev) % dtype_size(plan->dtype) || reinterpret_cast<uintptr_t>(out_dev) % 8)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: the array must be aligned to its element size, the result to 8 bytes");
    return est_reduce_launch(plan->g, plan->op, plan->dtype, in_dev, plan->ws.p, out_dev, as_stream(stream));
}

int mdsp_est_reduce_emulate(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments,
                            int64_t phase, int64_t* depth_reached) {
    bool empty = false;
    MDSP_TRY(est_check_shape(inner, len, outer, op, dtype, segments, &empty));
    if (phase < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_reduce: phase must be >= 0");
    if (depth_reached) *depth_reached = 0;
    if (empty) return MDSP_OK;
    if (!out_host || (!in_host && len > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const rop::Geom g = est_geometry(inner, len, outer, op, dtype, segments);
#define MDSP_EST_EMULATE(Op, T) est_emulate_as<Op, T>(in_host, out_host, g, phase, depth_reached)
    MDSP_EST_DISPATCH(op, dtype, MDSP_EST_EMULATE)
#undef MDSP_EST_EMULATE
    return MDSP_OK;
}

int mdsp_est_peak_gather(const void* bins_dev, int64_t nbins, int64_t n, int onesided, int dtype, const void* argmax_dev, void* out_dev, void* stream) {
    MDSP_TRY(peak_check(nbins, n, onesided, dtype, bins_dev, argmax_dev, out_dev));
    if (reinterpret_cast<uintptr_t>(bins_dev) % dtype_size(dtype) || reinterpret_cast<uintptr_t>(argmax_dev) % 8 || reinterpret_cast<uintptr_t>(out_dev) % 8)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "est_peak: the bins must be aligned to their element size, the records to 8 bytes");
    const int64_t* am = static_cast<const int64_t*>(argmax_dev);
    if (dtype == MDSP_C32) hipLaunchKernelGGL((peak_gather_kernel<rop::c32>), dim3(1), dim3(64), 0, as_stream(stream), static_cast<const rop::c32*>(bins_dev), nbins, n, onesided, am, out_dev);
    else hipLaunchKernelGGL((peak_gather_kernel<rop::c64>), dim3(1), dim3(64), 0, as_stream(stream), static_cast<const rop::c64*>(bins_dev), nbins, n, onesided, am, out_dev);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

int mdsp_est_peak_emulate(const void* bins_host, int64_t nbins, int64_t n, int onesided, int dtype, const void* argmax_host, void* out_host) {
    MDSP_TRY(peak_check(nbins, n, onesided, dtype, bins_host, argmax_host, out_host));
    const int64_t* am = static_cast<const int64_t*>(argmax_host);
    if (dtype == MDSP_C32) eop::peak_record<rop::c32>(static_cast<const rop::c32*>(bins_host), nbins, n, onesided, am, out_host);
    else eop::peak_record<rop::c64>(static_cast<const rop::c64*>(bins_host), nbins, n, onesided, am, out_host);
    return MDSP_OK;
}

int mdsp_quinn_geometry_for(int dtype, int64_t n, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run, int64_t* workspace_bytes) {
    MDSP_TRY(quinn_check(dtype, n, segments));
    const Geom g = make_geometry(dtype_is_complex(dtype), n, segments);
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (tile) *tile = TILE;
    if (run) *run = RUN;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_quinn_plan_create(mdsp_quinn_plan* plan, int dtype, int64_t n, int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    MDSP_TRY(quinn_check(dtype, n, segments));
    auto pl = new mdsp_quinn_plan_s();
    pl->g = make_geometry(dtype_is_complex(dtype), n, segments);
    pl->dtype = dtype;
    pl->gsum = est_geometry(1, n, 1, eop::OP_SUM, dtype, 0);
    *plan = pl;
    return MDSP_OK;
}

int mdsp_quinn_plan_destroy(mdsp_quinn_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_quinn_plan_info(mdsp_quinn_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (tile) *tile = TILE;
    if (run) *run = RUN;
    if (workspace_bytes) *workspace_bytes = plan->g.workspace;
    return MDSP_OK;
}

int mdsp_quinn_pass_exec(mdsp_quinn_plan plan, const void* x_dev, const double* mean, double param, void* out_dev, void* stream) {
    MDSP_TRY(exec_check(plan, x_dev));
    if (!mean || !out_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: NULL buffer");
    if (reinterpret_cast<uintptr_t>(out_dev) % 8) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: the record must be aligned to 8 bytes");
    MDSP_TRY(ensure_device(plan));
    return pass_exec(plan, x_dev, mean, param, static_cast<double*>(out_dev), as_stream(stream));
}

int mdsp_quinn_pass_emulate_host(const void* x_host, int dtype, int64_t n, int64_t segments, const double* mean, double param, double* out_host) {
    MDSP_TRY(quinn_check(dtype, n, segments));
    if (!x_host || !mean || !out_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: NULL buffer");
    const Geom g = make_geometry(dtype_is_complex(dtype), n, segments);
    if (g.cplx) {
        Pass<true> ps;
        MDSP_TRY(make_pass<true>(g, param, mean, &ps));
        if (dtype == MDSP_C32) emulate<true, rop::c32>(ps, g, static_cast<const rop::c32*>(x_host), out_host);
        else emulate<true, rop::c64>(ps, g, static_cast<const rop::c64*>(x_host), out_host);
    } else {
        Pass<false> ps;
        MDSP_TRY(make_pass<false>(g, param, mean, &ps));
        if (dtype == MDSP_F32) emulate<false, float>(ps, g, static_cast<const float*>(x_host), out_host);
        else emulate<false, double>(ps, g, static_cast<const double*>(x_host), out_host);
    }
    return MDSP_OK;
}

int mdsp_quinn_estimate(mdsp_quinn_plan plan, const void* x_dev, double f0, double fs, double tol, int64_t maxiters, double* estimate, int* reached_maxiters,
                        int64_t* iterations, void* stream) {
    MDSP_TRY(exec_check(plan, x_dev));
    if (!estimate || !reached_maxiters) MDSP_FAIL(MDSP_ERR_ARGUMENT, "quinn: NULL result");
    MDSP_TRY(ensure_device(plan));
    hipStream_t st = as_stream(stream);
    const Geom& g = plan->g;
    double* dev = plan->rec.as<double>();
    double rec[4] = {0.0, 0.0, 0.0, 0.0};
    // mean(x) (:164, :196): one SUM reduction, one small copy
    MDSP_TRY(est_reduce_launch(plan->gsum, eop::OP_SUM, plan->dtype, x_dev, plan->sumws.p, dev, st));
    MDSP_HIP(hipMemcpyAsync(rec, dev, (g.cplx ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    MDSP_HIP(hipStreamSynchronize(st));
    const double mean[2] = {rec[0] / (double)g.n, g.cplx ? rec[1] / (double)g.n : 0.0};
    const double nan = std::nan(""), pi = 3.14159265358979323846;
    const double fn = fs / 2;
    double w = pi * f0 / fn;
    int64_t iter = 0;
    // one pass and one small copy with a synchronisation; a parameter that is not finite gives a NaN record without a launch (a NaN runs to maxiters)
    auto run_pass = [&](double param) -> int {
        if (!std::isfinite(param)) {
            rec[0] = rec[1] = rec[2] = rec[3] = nan;
            return MDSP_OK;
        }
        MDSP_TRY(pass_exec(plan, x_dev, mean, param, dev + 2, st));
        MDSP_HIP(hipMemcpyAsync(rec, dev + 2, (g.cplx ? 3 : 4) * sizeof(double), hipMemcpyDeviceToHost, st));
        MDSP_HIP(hipStreamSynchronize(st));
        return MDSP_OK;
    };
    if (!g.cplx) {
        double alpha = 2 * std::cos(w), beta = 0.0;                 // :168-169
        for (int64_t it = 1; it <= maxiters; ++it) {                // :175-185
            iter = it;
            MDSP_TRY(run_pass(alpha));
            beta = (rec[3] / rec[2] + rec[0]) / rec[1];
            if (std::fabs(alpha - beta) < tol) break;
            alpha = 2 * beta - alpha;
        }
        if (std::fabs(0.5 * beta) > 1.0) MDSP_FAIL(MDSP_ERR_DOMAIN, "quinn: acos(%.17g): the iteration left [-1, 1]", 0.5 * beta);   // :187, acos throws
        *estimate = fn * std::acos(0.5 * beta) / pi;
    } else {
        for (int64_t it = 1; it <= maxiters; ++it) {                // :204-217
            iter = it;
            MDSP_TRY(run_pass(w));
            const double num = rec[1] * std::cos(w) - rec[0] * std::sin(w);   // imag(S conj(cis(w)))
            const double step = 2 * num / rec[2];
            w += step;
            if (std::fabs(step) < tol) break;
        }
        *estimate = fn * w / pi;
    }
    *reached_maxiters = iter == maxiters ? 1 : 0;
    if (iterations) *iterations = iter;
    return MDSP_OK;
}

}  // extern "C"
