// freqresp / phaseresp / grpdelay (Filters/response.jl:27-52, :73-76, :96-111) on the device.  The arithmetic, the forms and the geometry are resp_op.h
// (shared with the host emulation); here are the thread mapping and the C ABI.
//
// A lane per evaluation point, one wavefront per workgroup, nothing shared between lanes.  Where the coefficients come from, per form:
//   POLY      global memory at wave-uniform addresses: every lane of a wavefront needs coefficient k at the same step, so one scalar load serves all 64
//             (as sos.hip reads its matrices); the vectors have any length, which rules out kernel arguments, and staging them in LDS would add a copy
//             and a barrier for nothing a scalar load does not already give.
//   SECTIONS  the kernel arguments (at most 16 x 5 values and the gain, by value): wave-uniform by construction, no plan-owned device memory at all.
//   ZPK       global memory at wave-uniform addresses, as POLY: root lists are short but of any length.
// POLY with C > 1 is two launches on the caller's stream: (point tiles x chunks) workgroups store every chunk's value into the plan's workspace
// ([polynomial][chunk][point], consecutive lanes on consecutive words), then a lane per point forms q = y^L, runs Horner over the chunks, divides and
// stores.  Store first, sum afterwards: no atomics, no flags, nothing waits, and a result depends on the call's arguments only.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "resp_op.h"

using namespace mdsp;
using namespace mdsp::resp;

namespace {

template <typename R> struct Io {
    const void* in;     // IN_W: R[nw]; IN_POINTS: Cx<R>[nw]
    void* out;          // OUT_COMPLEX: Cx<R>[nw]; otherwise R[nw]
    int64_t nw;
    R cminus;
    int in_mode, neg, out_mode;
};

__device__ __forceinline__ void sincos_w(float w, float* s, float* c) { sincosf(w, s, c); }
__device__ __forceinline__ void sincos_w(double w, double* s, double* c) { sincos(w, s, c); }
__device__ __forceinline__ float atan2_w(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double atan2_w(double y, double x) { return atan2(y, x); }

template <typename R> __device__ __forceinline__ Cx<R> point(const Io<R>& io, int64_t i) {
    if (io.in_mode == IN_POINTS) return static_cast<const Cx<R>*>(io.in)[i];
    R s, c;
    sincos_w(static_cast<const R*>(io.in)[i], &s, &c);
    Cx<R> y;
    y.re = c;
    y.im = io.neg ? -s : s;
    return y;
}

template <typename R> __device__ __forceinline__ void store(const Io<R>& io, int64_t i, Cx<R> H) {
    if (io.out_mode == OUT_COMPLEX) static_cast<Cx<R>*>(io.out)[i] = H;
    else if (io.out_mode == OUT_ANGLE) static_cast<R*>(io.out)[i] = atan2_w(H.im, H.re);
    else static_cast<R*>(io.out)[i] = sub_rn(H.re, io.cminus);
}

template <typename R> struct PolyArgs {
    Io<R> io;
    const R* num;
    const R* den;       // nullptr: absent
    int64_t nnum, nden, C, L, tiles;
    Cx<R>* ws;          // C > 1: [polynomial][chunk][point]
    int log2L;
};

// C == 1: the whole thing.  C > 1: workgroup (tile, chunk) stores its chunk's values.
template <typename R, bool DERIV> __global__ __launch_bounds__(LANES) void resp_poly_kernel(const PolyArgs<R> a) {
    const int64_t tile = (int64_t)blockIdx.x % a.tiles, c = (int64_t)blockIdx.x / a.tiles;   // wave-uniform
    const int64_t i = tile * LANES + threadIdx.x;
    if (i >= a.io.nw) return;
    const Cx<R> y = point(a.io, i);
    const int64_t lo = c * a.L;
    const int64_t hin = std::min(lo + a.L, a.nnum), hid = std::min(lo + a.L, a.nden);
    const Cx<R> pn = poly_chunk<R, DERIV>(a.num, lo, hin, y);
    if (a.C == 1) {
        store(a.io, i, a.den ? cdiv(pn, poly_chunk<R, false>(a.den, lo, hid, y)) : pn);
        return;
    }
    a.ws[c * a.io.nw + i] = pn;
    if (a.den) a.ws[(a.C + c) * a.io.nw + i] = poly_chunk<R, false>(a.den, lo, hid, y);
}

template <typename R> __global__ __launch_bounds__(LANES) void resp_poly_finish_kernel(const PolyArgs<R> a) {
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= a.io.nw) return;
    const Cx<R> q = pow2l(point(a.io, i), a.log2L);
    const Cx<R> pn = chunk_horner(a.ws + i, a.io.nw, a.C, q);
    store(a.io, i, a.den ? cdiv(pn, chunk_horner(a.ws + a.C * a.io.nw + i, a.io.nw, a.C, q)) : pn);
}

template <typename R> struct SecArgs {
    Io<R> io;
    R c[5 * MAXK];
    R g;
    int K;
};
template <typename R> __global__ __launch_bounds__(LANES) void resp_sections_kernel(const SecArgs<R> a) {
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= a.io.nw) return;
    store(a.io, i, sections_value(a.c, a.K, a.g, point(a.io, i)));
}

template <typename R> struct ZpkArgs {
    Io<R> io;
    const Cx<R>* z;
    const Cx<R>* p;
    int64_t nz, np;
    R k;
};
template <typename R> __global__ __launch_bounds__(LANES) void resp_zpk_kernel(const ZpkArgs<R> a) {
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= a.io.nw) return;
    store(a.io, i, zpk_value(a.z, a.nz, a.p, a.np, a.k, point(a.io, i)));
}

constexpr int64_t MAX_GRID = 0x7fffffff;   // workgroups per launch

// what a plan and the emulation share: the checked arguments, the coefficients as the kernels use them (rounded to R, kept as doubles)
struct Spec {
    int form = FORM_POLY, flags = 0, out_mode = OUT_COMPLEX, in_mode = IN_POINTS, dtype = MDSP_F64;
    std::vector<double> num, den;   // POLY: b, a; SECTIONS: K x 5 in num; ZPK: (re, im) pairs of the zeros, of the poles
    int64_t nnum = 0, nden = 0, nw = 0;
    bool has_den = false, shared = false;   // shared: den is num itself (one device array)
    double gain = 1.0, cminus = 0.0;
    Geom g;
};

int check_args(int form, int flags, int out_mode, int in_mode, int dtype, const double* num, int64_t nnum, const double* den, int64_t nden, double gain,
               double cminus, int64_t nw, int64_t chunks, Spec* s) {
    if (form != FORM_POLY && form != FORM_SECTIONS && form != FORM_ZPK) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: unknown form %d", form);
    if (flags & ~(FLAG_DERIV | FLAG_NEG)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: unknown flags %d", flags);
    if ((flags & FLAG_DERIV) && form != FORM_POLY) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: MDSP_RESP_DERIV belongs to the POLY form");
    if (out_mode != OUT_COMPLEX && out_mode != OUT_ANGLE && out_mode != OUT_REAL_MINUS) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: unknown output mode %d", out_mode);
    if (in_mode != IN_W && in_mode != IN_POINTS) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: unknown input mode %d", in_mode);
    if (dtype != MDSP_F32 && dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: dtype must be MDSP_F32 or MDSP_F64 (the real type of the working type), got %d", dtype);
    if (nnum < 0 || nden < 0 || nw < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: negative size (%lld, %lld, %lld)", (long long)nnum, (long long)nden, (long long)nw);
    if (chunks < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: chunks must be >= 0 (0 = auto), got %lld", (long long)chunks);
    if ((nnum > 0 && !num) || (nden > 0 && !den)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: a coefficient array is NULL");
    if (form == FORM_POLY && nnum < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: the POLY form needs at least one numerator coefficient");
    if (form == FORM_SECTIONS && nden != 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: the SECTIONS form takes one table (nden must be 0)");
    if (form == FORM_SECTIONS && nnum > MAXK)
        MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "resp: cascades of more than %d sections are not accelerated (got %lld): use DSP.jl's CPU path", MAXK, (long long)nnum);
    if (nnum > (INT64_MAX >> 8) || nden > (INT64_MAX >> 8) || nw > (INT64_MAX >> 8)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: array too large");
    const bool dbl = dtype == MDSP_F64;
    auto rounded = [&](double v) { return dbl ? v : (double)(float)v; };
    const int64_t per = form == FORM_POLY ? 1 : form == FORM_SECTIONS ? 5 : 2;
    for (int64_t i = 0; i < per * nnum; ++i)
        if (!std::isfinite(rounded(num[i]))) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: value %lld of the first coefficient array is not finite", (long long)i);
    for (int64_t i = 0; i < per * nden; ++i)
        if (!std::isfinite(rounded(den[i]))) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: value %lld of the second coefficient array is not finite", (long long)i);
    if (!std::isfinite(rounded(gain)) || !std::isfinite(rounded(cminus))) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: the gain or the constant is not finite");
    s->form = form;
    s->flags = flags;
    s->out_mode = out_mode;
    s->in_mode = in_mode;
    s->dtype = dtype;
    s->nnum = nnum;
    s->nden = nden;
    s->nw = nw;
    s->has_den = form == FORM_POLY && nden > 0;
    s->shared = s->has_den && den == num && nden == nnum;
    s->gain = rounded(gain);
    s->cminus = rounded(cminus);
    s->num.resize((size_t)(per * nnum));
    s->den.resize((size_t)(per * nden));
    for (int64_t i = 0; i < per * nnum; ++i) s->num[(size_t)i] = rounded(num[i]);
    for (int64_t i = 0; i < per * nden; ++i) s->den[(size_t)i] = rounded(den[i]);
    s->g = make_geometry(form, dbl, std::max(nnum, nden), s->has_den, nw, chunks);
    const int64_t tiles = cdiv(nw, LANES);
    int64_t blocks = 0, wsb = 0;
    if (__builtin_mul_overflow(tiles, s->g.C, &blocks) || blocks > MAX_GRID) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: %lld points in %lld chunks exceed one launch", (long long)nw, (long long)s->g.C);
    if (s->g.C > 1 && (__builtin_mul_overflow(s->g.C * (s->has_den ? 2 : 1) * (dbl ? 16 : 8), nw, &wsb) || wsb != s->g.workspace)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: workspace too large");
    return MDSP_OK;
}

template <typename R> std::vector<R> as_type(const std::vector<double>& v) {
    std::vector<R> r(v.size());
    for (size_t i = 0; i < v.size(); ++i) r[i] = (R)v[i];
    return r;
}

inline float atan2_host(float y, float x) { return std::atan2(y, x); }
inline double atan2_host(double y, double x) { return std::atan2(y, x); }

template <typename R> void emulate(const Spec& s, const void* points, void* out) {
    const std::vector<R> num = as_type<R>(s.num), den = as_type<R>(s.den);
    const Cx<R>* pts = static_cast<const Cx<R>*>(points);
    const Geom& g = s.g;
    const int64_t nw = s.nw;
    std::vector<Cx<R>> ws((size_t)(g.C > 1 ? (s.has_den ? 2 : 1) * g.C * nw : 0));
    const bool deriv = (s.flags & FLAG_DERIV) != 0;
    auto put = [&](int64_t i, Cx<R> H) {
        if (s.out_mode == OUT_COMPLEX) static_cast<Cx<R>*>(out)[i] = H;
        else if (s.out_mode == OUT_ANGLE) static_cast<R*>(out)[i] = atan2_host(H.im, H.re);
        else static_cast<R*>(out)[i] = sub_rn(H.re, (R)s.cminus);
    };
    if (s.form == FORM_SECTIONS) {
        for (int64_t i = 0; i < nw; ++i) put(i, sections_value(num.data(), (int)s.nnum, (R)s.gain, pts[i]));
        return;
    }
    if (s.form == FORM_ZPK) {
        for (int64_t i = 0; i < nw; ++i)
            put(i, zpk_value(reinterpret_cast<const Cx<R>*>(num.data()), s.nnum, reinterpret_cast<const Cx<R>*>(den.data()), s.nden, (R)s.gain, pts[i]));
        return;
    }
    auto chunk_num = [&](int64_t lo, int64_t hi, Cx<R> y) { return deriv ? poly_chunk<R, true>(num.data(), lo, hi, y) : poly_chunk<R, false>(num.data(), lo, hi, y); };
    for (int64_t c = 0; c < g.C; ++c) {          // first launch: every (tile, chunk)
        const int64_t lo = c * g.L, hin = std::min(lo + g.L, s.nnum), hid = std::min(lo + g.L, s.nden);
        for (int64_t i = 0; i < nw; ++i) {
            const Cx<R> pn = chunk_num(lo, hin, pts[i]);
            if (g.C == 1) {
                put(i, s.has_den ? cdiv(pn, poly_chunk<R, false>(den.data(), lo, hid, pts[i])) : pn);
                continue;
            }
            ws[(size_t)(c * nw + i)] = pn;
            if (s.has_den) ws[(size_t)((g.C + c) * nw + i)] = poly_chunk<R, false>(den.data(), lo, hid, pts[i]);
        }
    }
    if (g.C == 1) return;
    for (int64_t i = 0; i < nw; ++i) {           // second launch
        const Cx<R> q = pow2l(pts[i], g.log2L);
        const Cx<R> pn = chunk_horner(ws.data() + i, nw, g.C, q);
        put(i, s.has_den ? cdiv(pn, chunk_horner(ws.data() + g.C * nw + i, nw, g.C, q)) : pn);
    }
}

int check_io(const Spec& s, const void* in, const void* out, bool host) {
    if (!in || !out) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: NULL buffer");
    const uintptr_t rs = s.dtype == MDSP_F64 ? 8 : 4;
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t ab = (uintptr_t)s.nw * rs * (s.in_mode == IN_POINTS ? 2 : 1), bb = (uintptr_t)s.nw * rs * (s.out_mode == OUT_COMPLEX ? 2 : 1);
    if (a < b + bb && b < a + ab) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: the output must not overlap the input");
    if (!host && (a % rs || b % rs)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: arrays must be aligned to their real element size");
    return MDSP_OK;
}

}  // namespace

struct mdsp_resp_plan_s {
    Spec s;
    std::mutex mu;
    bool on_device = false;   // the plan touches the device at its first exec, not before
    DevBuf dnum, dden, ws;
};

namespace {

template <typename R> int upload(DevBuf* buf, const std::vector<double>& v) {
    if (v.empty()) return MDSP_OK;
    const std::vector<R> t = as_type<R>(v);
    MDSP_TRY(buf->reserve(t.size() * sizeof(R)));
    MDSP_HIP(hipMemcpy(buf->p, t.data(), t.size() * sizeof(R), hipMemcpyHostToDevice));
    return MDSP_OK;
}

template <typename R> int ensure_device(mdsp_resp_plan pl) {
    std::lock_guard<std::mutex> lock(pl->mu);
    if (pl->on_device) return MDSP_OK;
    const Spec& s = pl->s;
    if (s.form != FORM_SECTIONS) {
        MDSP_TRY(upload<R>(&pl->dnum, s.num));
        if (!s.shared) MDSP_TRY(upload<R>(&pl->dden, s.den));
    }
    if (s.g.workspace > 0) MDSP_TRY(pl->ws.reserve((size_t)s.g.workspace));
    pl->on_device = true;
    return MDSP_OK;
}

template <typename R> int resp_exec(mdsp_resp_plan pl, const void* in, void* out, hipStream_t st) {
    MDSP_TRY(ensure_device<R>(pl));
    const Spec& s = pl->s;
    Io<R> io{};
    io.in = in;
    io.out = out;
    io.nw = s.nw;
    io.cminus = (R)s.cminus;
    io.in_mode = s.in_mode;
    io.neg = (s.flags & FLAG_NEG) ? 1 : 0;
    io.out_mode = s.out_mode;
    const int64_t tiles = cdiv(s.nw, LANES);
    const dim3 block(LANES);
    if (s.form == FORM_SECTIONS) {
        SecArgs<R> a{};
        a.io = io;
        for (int i = 0; i < 5 * MAXK; ++i) a.c[i] = i < 5 * s.nnum ? (R)s.num[(size_t)i] : (R)0;
        a.g = (R)s.gain;
        a.K = (int)s.nnum;
        hipLaunchKernelGGL((resp_sections_kernel<R>), dim3((unsigned)tiles), block, 0, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    if (s.form == FORM_ZPK) {
        ZpkArgs<R> a{};
        a.io = io;
        a.z = pl->dnum.as<Cx<R>>();
        a.p = pl->dden.as<Cx<R>>();
        a.nz = s.nnum;
        a.np = s.nden;
        a.k = (R)s.gain;
        hipLaunchKernelGGL((resp_zpk_kernel<R>), dim3((unsigned)tiles), block, 0, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    PolyArgs<R> a{};
    a.io = io;
    a.num = pl->dnum.as<R>();
    a.den = s.has_den ? (s.shared ? pl->dnum.as<R>() : pl->dden.as<R>()) : nullptr;
    a.nnum = s.nnum;
    a.nden = s.nden;
    a.C = s.g.C;
    a.L = s.g.L;
    a.tiles = tiles;
    a.ws = pl->ws.as<Cx<R>>();
    a.log2L = s.g.log2L;
    const dim3 grid((unsigned)(tiles * s.g.C));
    if (s.flags & FLAG_DERIV) hipLaunchKernelGGL((resp_poly_kernel<R, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((resp_poly_kernel<R, false>), grid, block, 0, st, a);
    MDSP_LAUNCH_CHECK();
    if (s.g.C > 1) {
        hipLaunchKernelGGL((resp_poly_finish_kernel<R>), dim3((unsigned)tiles), block, 0, st, a);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_resp_geometry_for(int form, int dtype, int64_t ncoef, int has_den, int64_t nw, int64_t chunks, int64_t* nchunks, int64_t* chunk_len,
                           int64_t* workspace_bytes) {
    if (form != FORM_POLY && form != FORM_SECTIONS && form != FORM_ZPK) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: unknown form %d", form);
    if (dtype != MDSP_F32 && dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: dtype must be MDSP_F32 or MDSP_F64, got %d", dtype);
    if (ncoef < 0 || nw < 0 || ncoef > (INT64_MAX >> 8) || nw > (INT64_MAX >> 8)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: bad size (%lld, %lld)", (long long)ncoef, (long long)nw);
    if (chunks < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "resp: chunks must be >= 0 (0 = auto), got %lld", (long long)chunks);
    const Geom g = make_geometry(form, dtype == MDSP_F64, ncoef, has_den != 0, nw, chunks);
    if (nchunks) *nchunks = g.C;
    if (chunk_len) *chunk_len = g.L;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_resp_plan_create(mdsp_resp_plan* plan, int form, int flags, int out_mode, int in_mode, int dtype, const double* num, int64_t nnum,
                          const double* den, int64_t nden, double gain, double cminus, int64_t nw, int64_t chunks) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    Spec s;
    MDSP_TRY(check_args(form, flags, out_mode, in_mode, dtype, num, nnum, den, nden, gain, cminus, nw, chunks, &s));
    auto pl = new mdsp_resp_plan_s();
    pl->s = std::move(s);
    *plan = pl;
    return MDSP_OK;
}

int mdsp_resp_plan_destroy(mdsp_resp_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_resp_plan_info(mdsp_resp_plan plan, int64_t* nchunks, int64_t* chunk_len, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nchunks) *nchunks = plan->s.g.C;
    if (chunk_len) *chunk_len = plan->s.g.L;
    if (workspace_bytes) *workspace_bytes = plan->s.g.workspace;
    return MDSP_OK;
}

int mdsp_resp_exec(mdsp_resp_plan plan, const void* w_or_points_dev, void* out_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (plan->s.nw == 0) return MDSP_OK;
    MDSP_TRY(check_io(plan->s, w_or_points_dev, out_dev, false));
    hipStream_t st = as_stream(stream);
    return plan->s.dtype == MDSP_F64 ? resp_exec<double>(plan, w_or_points_dev, out_dev, st) : resp_exec<float>(plan, w_or_points_dev, out_dev, st);
}

int mdsp_resp_emulate_host(const void* points_host, void* out_host, int form, int flags, int out_mode, int dtype, const double* num, int64_t nnum,
                           const double* den, int64_t nden, double gain, double cminus, int64_t nw, int64_t chunks) {
    Spec s;
    MDSP_TRY(check_args(form, flags, out_mode, IN_POINTS, dtype, num, nnum, den, nden, gain, cminus, nw, chunks, &s));
    if (nw == 0) return MDSP_OK;
    MDSP_TRY(check_io(s, points_host, out_host, true));
    if (dtype == MDSP_F64) emulate<double>(s, points_host, out_host);
    else emulate<float>(s, points_host, out_host);
    return MDSP_OK;
}

}  // extern "C"
