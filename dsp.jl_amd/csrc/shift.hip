// shiftsignal / shiftsignal! (src/util.jl:357-395) on the device: y[i] = x[i - s] where that exists, else 0.  The kernels move elements of 4, 8 or 16
// bytes as words, so every element type is covered.  Routes, the HALO schedule and the argument why each is safe in place: shift_plan.h (shared with
// the host emulation); here are the kernels and the C ABI.
#include <algorithm>

#include "common.h"
#include "shift_plan.h"

using namespace mdsp;
using namespace mdsp::shiftplan;

namespace {

struct alignas(4) W4 { uint32_t a; };
struct alignas(8) W8 { uint64_t a; };
struct alignas(8) W16 { uint64_t a, b; };   // a ComplexF64 is aligned like a Float64

constexpr int64_t MAX_GRID = 1 << 20;

// DISJOINT: a thread per destination element, four elements (256 apart) per thread and round, all loads of a round before its stores; x[j] stands at
// src[j - src_off] (STAGED reads the workspace).  zero_src (in place): the reader of word j stores the zero there, the destination thread of j leaves
// it alone.
constexpr int PER_THREAD = 4;

template <typename E>
__global__ __launch_bounds__(256) void shift_disjoint_kernel(const E* src, E* y, int64_t l, int64_t s, int64_t d, int64_t src_off, int zero_src) {
    const int64_t step = (int64_t)gridDim.x * 256 * PER_THREAD;
    const E zero{};
    for (int64_t i0 = (int64_t)blockIdx.x * 256 * PER_THREAD + threadIdx.x; i0 < l; i0 += step) {
        E v[PER_THREAD];
        bool has[PER_THREAD];
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r) {
            const int64_t i = i0 + r * 256, j = i - s;
            has[r] = i < l && j >= 0 && j < l;
            v[r] = zero;
            if (has[r]) v[r] = src[j - src_off];
        }
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r) {
            const int64_t i = i0 + r * 256, j = i - s;
            if (i >= l) continue;
            if (has[r]) {
                y[i] = v[r];
                if (zero_src) y[j] = zero;
            } else if (!(zero_src && in_source(i, l, s, d))) y[i] = zero;
        }
    }
}

template <typename E> __global__ __launch_bounds__(256) void shift_copy_kernel(const E* src, E* dst, int64_t n) {
    const int64_t step = (int64_t)gridDim.x * 256 * PER_THREAD;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 * PER_THREAD + threadIdx.x; i0 < n; i0 += step) {
        E v[PER_THREAD];
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r)
            if (i0 + r * 256 < n) v[r] = src[i0 + r * 256];
#pragma unroll
        for (int r = 0; r < PER_THREAD; ++r)
            if (i0 + r * 256 < n) dst[i0 + r * 256] = v[r];
    }
}

// HALO launch 1: nothing of the line is written here
template <typename E> __global__ __launch_bounds__(256) void shift_halo_kernel(const E* x, E* ws, int64_t l, int64_t s, int64_t d, int64_t tile, int64_t n) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += step) {
        const int64_t j = halo_word(g / d, g % d, s, d, tile);
        if (j >= 0 && j < l) ws[g] = x[j];
    }
}

// HALO launch 2: a workgroup per tile, chunk after chunk: load, wait for the loads, barrier, store
template <typename E>
__global__ __launch_bounds__(256) void shift_tile_kernel(E* x, const E* ws, int64_t l, int64_t s, int64_t d, int64_t tile, int64_t chunk, int64_t ntiles) {
    constexpr int R = (int)(CHUNK_MAX / 256);
    const E zero{};
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * tile, t1 = t0 + tile < l ? t0 + tile : l;
        for (int64_t c = 0; c * chunk < t1 - t0; ++c) {
            int64_t d0, d1;
            chunk_range(c, t0, t1, s, chunk, &d0, &d1);
            E v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = d0 + r * 256 + threadIdx.x;
                v[r] = zero;
                if (i < d1) {
                    int64_t idx = 0;
                    const int kind = source_of(i, t, l, s, d, tile, &idx);
                    if (kind == SRC_LINE) v[r] = x[idx];
                    else if (kind == SRC_HALO) v[r] = ws[idx];
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every load of this wavefront has returned ...
            __syncthreads();                                    // ... and of every other one of the workgroup, before the first store of the chunk
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = d0 + r * 256 + threadIdx.x;
                if (i < d1) x[i] = v[r];
            }
        }
    }
}

unsigned grid_for(int64_t n, int per_thread = 1) { return (unsigned)std::max<int64_t>(1, std::min(cdiv(n, 256 * per_thread), MAX_GRID)); }

int plan_for(int64_t l, int64_t s, int64_t esize, int in_place, int64_t tile, int route, Plan* p) {
    const char* why = "";
    const int st = make_plan(l, s, esize, in_place != 0, tile, route, p, &why);
    if (st == PLAN_DOMAIN) MDSP_FAIL(MDSP_ERR_DOMAIN, "%s (s = %lld, length %lld)", why, (long long)s, (long long)l);
    if (st != PLAN_OK) MDSP_FAIL(MDSP_ERR_ARGUMENT, "%s", why);
    if (l > (INT64_MAX >> 6)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "shift: line too long");
    return MDSP_OK;
}

}  // namespace

struct mdsp_shift_plan_s {
    Plan p;
    DevBuf ws;
};

namespace {

template <typename E> int shift_exec(mdsp_shift_plan pl, const void* in_dev, void* out_dev, hipStream_t st) {
    const Plan& p = pl->p;
    const E* x = static_cast<const E*>(in_dev);
    E* y = static_cast<E*>(out_dev);
    E* ws = pl->ws.as<E>();
    const dim3 block(256);
    if (p.route == ROUTE_DISJOINT) {
        hipLaunchKernelGGL((shift_disjoint_kernel<E>), dim3(grid_for(p.l, PER_THREAD)), block, 0, st, x, y, p.l, p.s, p.d, (int64_t)0, p.in_place ? 1 : 0);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    if (p.route == ROUTE_STAGED) {
        const int64_t b = source_begin(p.s, p.d), n = p.l - p.d;
        if (n > 0) {
            hipLaunchKernelGGL((shift_copy_kernel<E>), dim3(grid_for(n, PER_THREAD)), block, 0, st, x + b, ws, n);
            MDSP_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL((shift_disjoint_kernel<E>), dim3(grid_for(p.l, PER_THREAD)), block, 0, st, static_cast<const E*>(ws), y, p.l, p.s, p.d, b, 0);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    const int64_t n = p.ntiles * p.d;
    hipLaunchKernelGGL((shift_halo_kernel<E>), dim3(grid_for(n)), block, 0, st, x, ws, p.l, p.s, p.d, p.tile, n);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((shift_tile_kernel<E>), dim3((unsigned)std::min(p.ntiles, MAX_GRID)), block, 0, st, y, static_cast<const E*>(ws), p.l, p.s, p.d, p.tile,
                       p.chunk, p.ntiles);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_shift_geometry_for(int64_t l, int64_t s, int64_t elem_bytes, int in_place, int64_t tile, int route, int* route_out, int64_t* tile_out,
                            int64_t* chunk, int64_t* ntiles, int64_t* workspace_bytes) {
    Plan p;
    MDSP_TRY(plan_for(l, s, elem_bytes, in_place, tile, route, &p));
    if (route_out) *route_out = p.route;
    if (tile_out) *tile_out = p.tile;
    if (chunk) *chunk = p.chunk;
    if (ntiles) *ntiles = p.ntiles;
    if (workspace_bytes) *workspace_bytes = p.workspace * p.esize;
    return MDSP_OK;
}

int mdsp_shift_plan_create(mdsp_shift_plan* plan, int64_t l, int64_t s, int64_t elem_bytes, int in_place, int64_t tile, int route) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    Plan p;
    MDSP_TRY(plan_for(l, s, elem_bytes, in_place, tile, route, &p));
    auto pl = new mdsp_shift_plan_s();
    pl->p = p;
    if (p.workspace > 0) {
        const int st = pl->ws.reserve((size_t)(p.workspace * p.esize));
        if (st != MDSP_OK) {
            delete pl;
            return st;
        }
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_shift_plan_destroy(mdsp_shift_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_shift_plan_info(mdsp_shift_plan plan, int* route, int64_t* tile, int64_t* chunk, int64_t* ntiles, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (route) *route = plan->p.route;
    if (tile) *tile = plan->p.tile;
    if (chunk) *chunk = plan->p.chunk;
    if (ntiles) *ntiles = plan->p.ntiles;
    if (workspace_bytes) *workspace_bytes = (int64_t)plan->ws.bytes;
    return MDSP_OK;
}

int mdsp_shift_exec(mdsp_shift_plan plan, const void* in_dev, void* out_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    const Plan& p = plan->p;
    if (p.l == 0) return MDSP_OK;
    if (!in_dev || !out_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(in_dev), b = reinterpret_cast<uintptr_t>(out_dev), bytes = (uintptr_t)(p.l * p.esize);
    if ((a == b) != p.in_place) MDSP_FAIL(MDSP_ERR_ARGUMENT, "shift: the plan was made %s", p.in_place ? "in place: out must be the input" : "out of place: out must not be the input");
    if (a != b && a < b + bytes && b < a + bytes) MDSP_FAIL(MDSP_ERR_ARGUMENT, "shift: out must be the input array itself or not overlap it");
    const uintptr_t align = p.esize == 4 ? 4 : 8;
    if (a % align || b % align) MDSP_FAIL(MDSP_ERR_ARGUMENT, "shift: arrays must be aligned to their element size (ComplexF64: 8 bytes)");
    if (p.in_place && p.s == 0) return MDSP_OK;
    hipStream_t st = as_stream(stream);
    return p.esize == 4 ? shift_exec<W4>(plan, in_dev, out_dev, st) : p.esize == 8 ? shift_exec<W8>(plan, in_dev, out_dev, st) : shift_exec<W16>(plan, in_dev, out_dev, st);
}

int mdsp_shift_emulate(const void* in_host, void* out_host, int64_t l, int64_t s, int64_t elem_bytes, int64_t tile, int route, int order,
                       int64_t* violations) {
    Plan p;
    MDSP_TRY(plan_for(l, s, elem_bytes, in_host == out_host, tile, route, &p));
    if (order < 0 || order > 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "shift: order is 0, 1 or 2");
    if (violations) *violations = 0;
    if (l == 0) return MDSP_OK;
    if (!in_host || !out_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (elem_bytes == 4) emulate<W4>(p, static_cast<const W4*>(in_host), static_cast<W4*>(out_host), order, violations);
    else if (elem_bytes == 8) emulate<W8>(p, static_cast<const W8*>(in_host), static_cast<W8*>(out_host), order, violations);
    else emulate<W16>(p, static_cast<const W16*>(in_host), static_cast<W16*>(out_host), order, violations);
    return MDSP_OK;
}

}  // extern "C"
