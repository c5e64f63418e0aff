// arburg / lpc (src/lpc.jl:28-32, :53-92) on the device: Burg's lattice passes.  The arithmetic, the geometry, the order of every addition and the host
// emulation are burg_op.h; here are the thread mapping of a sweep, the finish and the C ABI.
//
// A sweep: a wavefront per segment, four per workgroup, nothing shared between wavefronts.  Lane l of a tile owns V = 16 bytes / sizeof(F) consecutive
// pairs: ef[i ..] and eb[i + m ..] are each one 16-byte load where the ADDRESS of the wavefront's first element is a multiple of 16 -- the tiles advance by
// 1024 bytes, so the answer is the same for every tile and every lane: a wave-uniform branch -- and V element loads otherwise (the eb side moves by one
// element per order: it is vector-aligned in one order of V).  Only full vectors inside the segment are loaded or stored as vectors; the ragged end goes
// element by element, and nothing outside [0, n) of either array is touched.  A lane reads and writes its own pairs only; the eb' of the next lane's
// first pair comes by a lane exchange, the ef' of a tile's last pair is carried to lane 0 of the next tile, and the product across a segment boundary is
// left to the finish, which reads both factors from the finished arrays behind a kernel boundary: no sweep reads what another wavefront writes.
#include <algorithm>
#include <mutex>

#include "burg_op.h"
#include "common.h"

using namespace mdsp;
using namespace mdsp::burg;
namespace rop = mdsp::reduceop;

namespace {

template <typename F> struct SweepArgs {
    int64_t n, S, seglen, m;
    const F* ein;     // m <= 1: x
    const F* bin;
    F* eout;          // m >= 1: the work arrays
    F* bout;
    const F* k;       // m >= 1: the reflection coefficient of this order, in the record
    Sums* part;       // S partials
};

template <typename F> struct FinishArgs {
    int64_t n, S, seglen, m, p;
    const F* ef;      // m <= 1: x
    const F* eb;
    const Sums* part;
    State<typename Elem<F>::R>* state;
    F* rec;
};

template <typename F> __device__ __forceinline__ F shfl_elem(F v, int src) {
    constexpr int W = (int)sizeof(F) / 4;
    int w[W];
    __builtin_memcpy(w, &v, sizeof(F));
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = __shfl(w[i], src, 64);
    __builtin_memcpy(&v, w, sizeof(F));
    return v;
}
template <typename F> __device__ __forceinline__ F shfl_down_elem(F v) {
    constexpr int W = (int)sizeof(F) / 4;
    int w[W];
    __builtin_memcpy(w, &v, sizeof(F));
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = __shfl_down(w[i], 1, 64);
    __builtin_memcpy(&v, w, sizeof(F));
    return v;
}

__device__ __forceinline__ Sums wave_fold_sums(Sums a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) a.s[i] = add_rn(a.s[i], __shfl_down(a.s[i], off, 64));
    }
    return a;
}

template <typename F> __device__ __forceinline__ void load_run(const F* p, int cnt, bool vec, F* v) {
    constexpr int V = Lane<F>::V;
    if (vec && cnt == V) {
        const uint4 w = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(v, &w, 16);
    } else {
#pragma unroll
        for (int t = 0; t < V; ++t)
            if (t < cnt) v[t] = p[t];
    }
}
template <typename F> __device__ __forceinline__ void store_run(F* p, int cnt, bool vec, const F* v) {
    constexpr int V = Lane<F>::V;
    if (vec && cnt == V) {
        uint4 w;
        __builtin_memcpy(&w, v, 16);
        *reinterpret_cast<uint4*>(p) = w;
    } else {
#pragma unroll
        for (int t = 0; t < V; ++t)
            if (t < cnt) p[t] = v[t];
    }
}

// UPDATE false: sweep 0 (x is read, nothing but the partial is written)
template <typename F, bool UPDATE> __global__ __launch_bounds__(256) void burg_sweep_kernel(const SweepArgs<F> a) {
    constexpr int V = Lane<F>::V;
    constexpr int TILE = Lane<F>::TILE;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    F k{};
    if (UPDATE) k = *a.k;
    for (int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); unit < a.S; unit += nwaves) {   // wave-uniform
        int64_t j0, j1;
        segment_range(a.n, a.S, a.seglen, unit, a.m, &j0, &j1);
        const bool evec = reinterpret_cast<uintptr_t>(a.ein + j0) % 16 == 0, bvec = reinterpret_cast<uintptr_t>(a.bin + j0 + a.m) % 16 == 0;
        const bool eovec = UPDATE && reinterpret_cast<uintptr_t>(a.eout + j0) % 16 == 0, bovec = UPDATE && reinterpret_cast<uintptr_t>(a.bout + j0 + a.m) % 16 == 0;
        Sums acc = OpSums::identity();
        F carry_e{};
        for (int64_t t0 = j0; t0 < j1; t0 += TILE) {   // wave-uniform
            const int64_t i = t0 + (int64_t)lane * V;
            const int64_t left = j1 - i;
            const int cnt = (int)(left < 0 ? 0 : left > V ? V : left);
            F e[V], b[V];
#pragma unroll
            for (int t = 0; t < V; ++t) e[t] = b[t] = F{};
            if (cnt > 0) {
                load_run<F>(a.ein + i, cnt, evec, e);
                load_run<F>(a.bin + i + a.m, cnt, bvec, b);
                if (UPDATE) {
                    lane_update<F>(k, e, b, cnt);
                    store_run<F>(a.eout + i, cnt, eovec, e);
                    store_run<F>(a.bout + i + a.m, cnt, bovec, b);
                }
            }
            const F next_b = shfl_down_elem<F>(b[0]);
            const bool has_next = lane < 63 && i + V < j1;
            lane_terms<F>(e, b, cnt, !UPDATE, lane == 0 && t0 > j0, carry_e, has_next, next_b, acc);
            carry_e = shfl_elem<F>(e[V - 1], 63);
        }
        acc = wave_fold_sums(acc);
        if (lane == 0) a.part[unit] = acc;
    }
}

// one wavefront: the partials, the boundary terms, the fold; then every lane takes the same scalar step and the lanes share the pairs of a
template <typename F> __global__ __launch_bounds__(64) void burg_finish_kernel(const FinishArgs<F> a) {
    using R = typename Elem<F>::R;
    const int lane = threadIdx.x & 63;
    const rop::Params prm{0.0, 0};
    Sums acc = rop::finish_walk<OpSums>(a.part, a.S, lane, prm);
    if (a.m >= 1) {
        for (int64_t s = lane; s + 1 < a.S; s += 64) {
            const int64_t ib = (s + 1) * a.seglen;
            if (ib < a.n - a.m + 1) add_term<F>(a.eb[ib + a.m - 1], a.ef[ib - 1], acc);
        }
    }
    acc = wave_fold_sums(acc);
#pragma unroll
    for (int i = 0; i < 3; ++i) acc.s[i] = __shfl(acc.s[i], 0, 64);
    State<R> st;
    if (a.m <= 1) state_init<F>(acc.s[2], a.n, st);
    else st = *a.state;
    if (a.m == 0) {   // p = 0
        if (lane == 0) {
            a.rec[0] = elem<F>((R)1, (R)0);
            a.rec[1] = elem<F>(st.err, (R)0);
        }
        return;
    }
    const F k = scalar_step<F>(acc.s[0], acc.s[1], a.ef[a.n - a.m], a.eb[a.m - 1], st);
    if (lane == 0) {
        *a.state = st;
        a.rec[a.p + a.m] = k;
        if (a.m == a.p) a.rec[2 * a.p + 1] = elem<F>(st.err, (R)0);
    }
    for (int64_t j = lane; j <= a.m / 2; j += 64) a_update_pair<F>(a.rec, a.m, j, k, a.m == 1, a.m == a.p);
}

constexpr int64_t MAX_SWEEP_GRID = 1 << 16;

int burg_check(int dtype, int64_t n, int64_t segments) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: bad dtype %d", dtype);
    if (n < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: at least one sample is needed (got %lld)", (long long)n);
    if (n > (INT64_MAX >> 6)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: signal too long");
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    return MDSP_OK;
}

int burg_check_order(int64_t n, int64_t p) {
    if (p < 0 || p > n - 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: the order must be in [0, n - 1] = [0, %lld], got %lld", (long long)(n - 1), (long long)p);
    return MDSP_OK;
}

template <typename F> int burg_launch(const Geom& g, const void* x_dev, int64_t p, void* ws, void* rec_dev, hipStream_t st) {
    using R = typename Elem<F>::R;
    const F* x = static_cast<const F*>(x_dev);
    F* rec = static_cast<F*>(rec_dev);
    const int64_t arr = (g.n * (int64_t)sizeof(F) + 255) / 256 * 256;
    char* w = static_cast<char*>(ws);
    F* ef = reinterpret_cast<F*>(w);
    F* eb = reinterpret_cast<F*>(w + arr);
    Sums* part = reinterpret_cast<Sums*>(w + 2 * arr);
    State<R>* state = reinterpret_cast<State<R>*>(w + 2 * arr + g.S * (int64_t)sizeof(Sums));
    const dim3 grid((unsigned)std::min(cdiv(g.S, 4), MAX_SWEEP_GRID)), block(256);
    SweepArgs<F> sa{g.n, g.S, g.seglen, 0, x, x, nullptr, nullptr, nullptr, part};
    hipLaunchKernelGGL((burg_sweep_kernel<F, false>), grid, block, 0, st, sa);
    MDSP_LAUNCH_CHECK();
    FinishArgs<F> fa{g.n, g.S, g.seglen, 0, p, x, x, part, state, rec};
    if (p == 0) {
        hipLaunchKernelGGL((burg_finish_kernel<F>), dim3(1), dim3(64), 0, st, fa);
        MDSP_LAUNCH_CHECK();
    }
    for (int64_t m = 1; m <= p; ++m) {
        fa.m = m;
        fa.ef = m == 1 ? x : ef;
        fa.eb = m == 1 ? x : eb;
        hipLaunchKernelGGL((burg_finish_kernel<F>), dim3(1), dim3(64), 0, st, fa);
        MDSP_LAUNCH_CHECK();
        if (m == p) break;   // the update after the last order is never used
        sa.m = m;
        sa.ein = fa.ef;
        sa.bin = fa.eb;
        sa.eout = ef;
        sa.bout = eb;
        sa.k = rec + p + m;
        hipLaunchKernelGGL((burg_sweep_kernel<F, true>), grid, block, 0, st, sa);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

}  // namespace

struct mdsp_burg_plan_s {
    Geom g;
    int dtype = MDSP_F32;
    std::mutex mu;
    DevBuf ws;   // the plan touches the device at its first exec, not before
};

extern "C" {

int mdsp_burg_geometry_for(int dtype, int64_t n, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* workspace_bytes) {
    MDSP_TRY(burg_check(dtype, n, segments));
    const Geom g = make_geometry((int64_t)dtype_size(dtype), n, segments);
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (tile) *tile = g.tile;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_burg_plan_create(mdsp_burg_plan* plan, int dtype, int64_t n, int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    MDSP_TRY(burg_check(dtype, n, segments));
    auto pl = new mdsp_burg_plan_s();
    pl->g = make_geometry((int64_t)dtype_size(dtype), n, segments);
    pl->dtype = dtype;
    *plan = pl;
    return MDSP_OK;
}

int mdsp_burg_plan_destroy(mdsp_burg_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_burg_plan_info(mdsp_burg_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (tile) *tile = plan->g.tile;
    if (workspace_bytes) *workspace_bytes = plan->g.workspace;
    return MDSP_OK;
}

int mdsp_burg_exec(mdsp_burg_plan plan, const void* x_dev, int64_t p, void* record_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    MDSP_TRY(burg_check_order(plan->g.n, p));
    if (!x_dev || !record_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: NULL buffer");
    const size_t es = dtype_size(plan->dtype);
    if (reinterpret_cast<uintptr_t>(x_dev) % es || reinterpret_cast<uintptr_t>(record_dev) % es)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: the signal and the record must be aligned to the element size");
    {
        std::lock_guard<std::mutex> lock(plan->mu);
        MDSP_TRY(plan->ws.reserve((size_t)plan->g.workspace));
    }
    hipStream_t st = as_stream(stream);
    switch (plan->dtype) {
        case MDSP_F32: return burg_launch<float>(plan->g, x_dev, p, plan->ws.p, record_dev, st);
        case MDSP_F64: return burg_launch<double>(plan->g, x_dev, p, plan->ws.p, record_dev, st);
        case MDSP_C32: return burg_launch<c32>(plan->g, x_dev, p, plan->ws.p, record_dev, st);
        default: return burg_launch<c64>(plan->g, x_dev, p, plan->ws.p, record_dev, st);
    }
}

int mdsp_burg_emulate_host(const void* x_host, int dtype, int64_t n, int64_t segments, int64_t p, void* record_host) {
    MDSP_TRY(burg_check(dtype, n, segments));
    MDSP_TRY(burg_check_order(n, p));
    if (!x_host || !record_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "burg: NULL buffer");
    const Geom g = make_geometry((int64_t)dtype_size(dtype), n, segments);
    switch (dtype) {
        case MDSP_F32: emulate<float>(g, static_cast<const float*>(x_host), p, static_cast<float*>(record_host)); break;
        case MDSP_F64: emulate<double>(g, static_cast<const double*>(x_host), p, static_cast<double*>(record_host)); break;
        case MDSP_C32: emulate<c32>(g, static_cast<const c32*>(x_host), p, static_cast<c32*>(record_host)); break;
        default: emulate<c64>(g, static_cast<const c64*>(x_host), p, static_cast<c64*>(record_host)); break;
    }
    return MDSP_OK;
}

}  // extern "C"
