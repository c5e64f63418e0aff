// Deterministic reductions along one dimension on the device (rms, rmsfft, meanfreq, finddelay of src/util.jl).  The operators, the geometry and the
// walk of a lane are reduce_op.h (shared with the host emulation, which therefore adds in the same order), the thread mappings and the launches
// reduce_kernels.h (shared with estimation.hip); here are the operators' dispatch and the C ABI.
#include <algorithm>
#include <vector>

#include "common.h"
#include "reduce_kernels.h"

using namespace mdsp;
using namespace mdsp::reduceop;

namespace {

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
    return launch_reduce<Op, T>(pl->g, pl->prm, in_dev, pl->ws.p, out_dev, st);
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
