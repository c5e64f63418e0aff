// Stateful polyphase FIR filtering / rational resampling (mdsp_fir_*): the generic kernel, the Float32 register-tap kernel, and the dispatch over every
// kernel family -- decimator (fir_dec.hip), matrix cores (fir_mm.hip), register taps for the other types (fir_reg.hip, fir_creg.hip).  FIRArbitrary lives
// in fir_arb.hip, the time-domain FIR (mdsp_tdfir_*) in tdfir.hip; the filter objects and the functions the units share are in fir_plan.h.
//
// Reference loop being replaced (src/Filters/stream_filt.jl:496-509, and its :409-428 / :452-463 / :541-552 twins):
//     while inputIdx <= xLen
//         y[bufIdx += 1] = unsafe_dot(pfb, phiIdx, (history,) x, inputIdx)      util.jl:225-283 (BLAS.dot per sample)
//         inputIdx += div(phiIdx + M - 1, L);  phiIdx = mod1(phiIdx + mod(M, L), L)
// The recurrence is serial; its closed form makes every output independent: for 0-based output m
//     p = (phi0 - 1) + m*M,   phi_m = p mod L (0-based column),   inputIdx_m = d0 + p div L (1-based, as the reference)
//     y[m] = sum_{i=0}^{tp-1} pfb[i, phi_m] * z[inputIdx_m - 1 + i],     z = [history (tp-1 samples) ; x]
// FIRStandard is L = M = 1, FIRDecimator L = 1, FIRInterpolator M = 1 (pfb = reversed taps for L = 1), so one
// kernel serves all four reference kernels.  phi0 / d0 / history are exactly the reference's state and are
// advanced on the host with the same integer arithmetic (bit-exact, see mdsp_fir_exec).
//
// Kernel: each workgroup produces a tile of consecutive outputs of one channel.  The input span of the tile
// (plus the tp-1 sample history halo) is staged once into LDS with coalesced loads, the transposed filter bank
// pfbT[i][phi] lives in LDS as well (phase index contiguous: lanes advance by M mod L phases per output, which
// spreads them over the banks), and every output is a tp-term fused multiply-add chain, oldest sample first.
#include <algorithm>
#include <numeric>
#include <vector>

#include "fir_plan.h"
#include "fir_op.h"
#include "fir_mm.h"
#include "fir_dec.h"
#include "fir_reg.h"
#include "fir_creg.h"
#include "hostpipe.h"
#include "devio.h"

using namespace mdsp;
using namespace mdsp::firop;
using mdsp::fft::cx;

namespace {

// XS: storage type of x (float, double, cx<float>, cx<double>);  A: accumulate/output type (R or cx<R>);  Z: staged type (A for real taps; under complex
// taps the signal's own class in the arithmetic precision, so a real signal takes half the LDS of its complex output);  H: tap type (R or cx<R>)
template <typename XS, typename A, typename R, typename Z = A, typename H = R>
MDSP_NO_LSO __global__ __launch_bounds__(256) void polyphase_fir_kernel(FirArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Z* zs = reinterpret_cast<Z*>(smem);                                  // staged input span (converted to Z)
    H* ps = reinterpret_cast<H*>(smem + (size_t)a.span * sizeof(Z));      // pfbT (optional)
    const int64_t ch = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * a.tile;
    if (m0 >= a.nout) return;
    const int cnt = (int)std::min<int64_t>(a.tile, a.nout - m0);
    const XS* xc = static_cast<const XS*>(a.x) + ch * a.ldx;
    const XS* hc = static_cast<const XS*>(a.hist) + ch * (int64_t)a.hl;
    // z-index range of the tile: first = inputIdx(m0) - 1, last = inputIdx(m0+cnt-1) - 1 + tp - 1
    const int64_t p_first = a.phi0m1 + m0 * a.M;
    const int64_t p_last = a.phi0m1 + (m0 + cnt - 1) * a.M;
    const int64_t z_first = a.d0 + p_first / a.L - 1;
    const int64_t z_last = a.d0 + p_last / a.L - 1 + a.tp - 1;
    const int nz = (int)(z_last - z_first + 1);
    for (int k = threadIdx.x; k < nz; k += blockDim.x) {
        const int64_t zi = z_first + k;  // index into [history ; x]
        Z v{};
        if (zi < a.hl) v = to_acc(hc[zi], (Z*)nullptr);
        else if (zi - a.hl < a.xlen) v = to_acc(xc[zi - a.hl], (Z*)nullptr);
        zs[k] = v;
    }
    const H* pf = static_cast<const H*>(a.pfbT);
    if (a.pfb_in_lds) {
        const int np = a.tp * a.L;
        for (int k = threadIdx.x; k < np; k += blockDim.x) ps[k] = pf[k];
        pf = ps;
    }
    __syncthreads();
    A* yc = static_cast<A*>(a.y) + ch * a.ldy;
    for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
        const int64_t p = p_first + (int64_t)j * a.M;
        const int phi = (int)(p % a.L);
        const int zoff = (int)(a.d0 + p / a.L - 1 - z_first);
        const Z* zp = zs + zoff;
        const H* hp = pf + phi;
        A acc = mul_first(hp[0], zp[0]);
        for (int i = 1; i < a.tp; ++i) fma_acc(acc, hp[(int64_t)i * a.L], zp[i]);
        yc[m0 + j] = acc;
    }
}

// history update (shiftin!, util.jl:299-314): new = last hl samples of [old ; x]
template <typename XS>
MDSP_NO_LSO __global__ __launch_bounds__(256) void shiftin_kernel(const XS* __restrict__ x, const XS* __restrict__ old, XS* __restrict__ neu, int64_t xlen,
                                                      int64_t ldx, int hl) {
    const int64_t ch = blockIdx.y;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < hl; k += gridDim.x * blockDim.x) {
        const int64_t zi = (int64_t)hl + xlen - hl + k;  // index into [old ; x] of new[k]  = xlen + k
        XS v;
        if (zi < hl) v = old[ch * hl + zi];
        else v = x[ch * ldx + (zi - hl)];
        neu[ch * hl + k] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Fast path (Float32 taps and real Float32 signal, tapsPerPhase <= 64): "a thread owns P consecutive output residues".
//
// Outputs m = q*L + s (round q, residue s) all use phase phi_s = (phi0-1 + s*M) mod L and the z-window that starts at
// q*M + c_s,  c_s = d0-1 + (phi0-1 + s*M) div L  -- both independent of q.  So a thread keeps the taps of its P residues
// in registers for the whole kernel, pre-shifted by delta_k = c_{s+k} - c_s (0 <= delta_k <= P-1 when M <= L), and per
// round reads ONE window of W = TPC+P-1 samples from LDS for its P outputs:  LDS reads per output drop from 2*tp
// (generic kernel: tap + sample) to W/P, and the FMA chain keeps the oldest-sample-first order.
// ------------------------------------------------------------------------------------------------------------
struct FirFastArgs {
    const float* x;
    const float* hist;
    float* y;
    const float* pfbT;   // tp * L
    int64_t xlen, ldx, ldy, nout, nrounds;
    int64_t phi0m1, d0;
    int L, M, tp, hl;
    int Q;               // rounds per tile
    int NP, RL;          // phase groups, round lanes (blockDim.x = NP * RL)
    int span;            // LDS floats per tile
    unsigned char gmap[256];   // thread -> phase group (a permutation of 0..NP-1 per round lane): see fir_lane_map
};

template <int TPC, int P>
MDSP_NO_LSO __global__ __launch_bounds__(256) void polyphase_fast_kernel(FirFastArgs a) {
    constexpr int W = TPC + P - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* zs = reinterpret_cast<float*>(smem);
    const int64_t ch = blockIdx.y;
    const int g = a.gmap[threadIdx.x], r = threadIdx.x / a.NP;
    const float* xc = a.x + ch * a.ldx;
    const float* hc = a.hist + ch * (int64_t)a.hl;
    float* yc = a.y + ch * a.ldy;
    // per-thread constants: offsets c_k (relative to c of residue 0 of the tile), shifted taps
    const int s0 = g * P;
    int coff[P];
    bool valid[P];
    float h[P][W];
    const int64_t cbase = a.d0 - 1;   // c_s = cbase + (phi0m1 + s*M) div L
    int c0rel = 0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int s = s0 + k;
        valid[k] = s < a.L;
        const int64_t p = a.phi0m1 + (int64_t)(valid[k] ? s : 0) * a.M;
        const int phi = (int)(p % a.L);
        const int crel = (int)(p / a.L);           // c_s - cbase
        if (k == 0) c0rel = crel;
        const int delta = valid[k] ? crel - c0rel : 0;   // 0..P-1 (M <= L)
        coff[k] = delta;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int i = j - delta;
            h[k][j] = (valid[k] && i >= 0 && i < a.tp) ? a.pfbT[(int64_t)i * a.L + phi] : 0.0f;
        }
    }
    (void)coff;
    const int64_t ntiles = (a.nrounds + a.Q - 1) / a.Q;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t q0 = tile * a.Q;
        const int nq = (int)std::min<int64_t>(a.Q, a.nrounds - q0);
        // z range of the tile: [q0*M + cbase, q0*M + cbase + nq*M + M + W)
        const int64_t z0 = q0 * a.M + cbase;
        const int nz = nq * a.M + a.M + W;
        __syncthreads();   // previous tile fully consumed
        if (z0 >= a.hl) {
            // steady state: the tile lies inside x.  Descriptor re-based at the tile start (hardware zero fill past the end
            // of the signal); 8 independent coalesced loads in flight per thread before the LDS writes.
            const float* src = xc + (z0 - a.hl);
            const __amdgpu_buffer_rsrc_t rs = io::make_rsrc(src, (a.xlen - (z0 - a.hl)) * 4);
            const int step = blockDim.x;
            for (int k2 = threadIdx.x; k2 < nz; k2 += 8 * step) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = io::Ld<float>::load(rs, (k2 + u * step) * 4);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (k2 + u * step < nz) zs[k2 + u * step] = v[u];
            }
        } else {  // the first tile(s) straddle the history
            for (int k2 = threadIdx.x; k2 < nz; k2 += blockDim.x) {
                const int64_t zi = z0 + k2;
                float v = 0.0f;
                if (zi < a.hl) v = hc[zi];
                else if (zi - a.hl < a.xlen) v = xc[zi - a.hl];
                zs[k2] = v;
            }
        }
        __syncthreads();
        if (valid[0]) {
            for (int q = r; q < nq; q += a.RL) {
                const float* zp = zs + q * a.M + c0rel;
                float acc[P];
                if constexpr (P == 2) {   // both residues in one v_pk_fma_f32 per tap (sample broadcast by op_sel)
                    typedef float f2v __attribute__((ext_vector_type(2)));
                    f2v a2 = {0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const float xv = zp[j];
                        a2 = __builtin_elementwise_fma(f2v{xv, xv}, f2v{h[0][j], h[1][j]}, a2);
                    }
                    acc[0] = a2.x;
                    acc[1] = a2.y;
                } else if constexpr (P == 4) {   // four residues: two packed FMAs per tap, W / 4 LDS reads per output instead of W / 2
                    typedef float f2v __attribute__((ext_vector_type(2)));
                    f2v a01 = {0.0f, 0.0f}, a23 = {0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const float xv = zp[j];
                        a01 = __builtin_elementwise_fma(f2v{xv, xv}, f2v{h[0][j], h[1][j]}, a01);
                        a23 = __builtin_elementwise_fma(f2v{xv, xv}, f2v{h[2][j], h[3][j]}, a23);
                    }
                    acc[0] = a01.x; acc[1] = a01.y; acc[2] = a23.x; acc[3] = a23.y;
                } else {
#pragma unroll
                    for (int k = 0; k < P; ++k) acc[k] = 0.0f;
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const float xv = zp[j];
#pragma unroll
                        for (int k = 0; k < P; ++k) acc[k] = fmaf(xv, h[k][j], acc[k]);
                    }
                }
                const int64_t m = (q0 + q) * a.L + s0;
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (valid[k] && m + k < a.nout) yc[m + k] = acc[k];
            }
        }
    }
}

int64_t gcd64(int64_t a, int64_t b) { return std::gcd(a, b); }

template <typename XS, typename A, typename R, typename Z = A, typename H = R> int fir_launch(mdsp_fir_s* f, FirArgs& a, hipStream_t st) {
    // tile size: keep the staged span + filter bank within 64 KiB of LDS
    const int64_t pfb_bytes = (int64_t)f->tp * f->L * (int64_t)sizeof(H);
    a.pfb_in_lds = pfb_bytes <= 40 * 1024;
    int tile = 4096;
    int64_t span = 0;
    while (true) {
        span = ((int64_t)tile * f->M + f->L - 1) / f->L + f->tp + 2;
        const int64_t bytes = span * (int64_t)sizeof(Z) + (a.pfb_in_lds ? pfb_bytes : 0);
        if (bytes <= 64 * 1024 || tile <= 64) break;
        tile /= 2;
    }
    // the smallest tile and the bank together miss the LDS (ComplexF64 decimation by 63 with 5000 taps: 144 + 40 KiB): the taps stay in L2
    if (a.pfb_in_lds && span * (int64_t)sizeof(Z) + pfb_bytes > 150 * 1024) a.pfb_in_lds = 0;
    const int64_t lds_bytes = span * (int64_t)sizeof(Z) + (a.pfb_in_lds ? pfb_bytes : 0);
    if (lds_bytes > 150 * 1024) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "filter too long for the polyphase kernel (tapsPerPhase=%lld)", (long long)f->tp);
    a.tile = tile;
    a.span = (int)span;
    auto kern = polyphase_fir_kernel<XS, A, R, Z, H>;
    if (lds_bytes > 48 * 1024) MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const dim3 grid((unsigned)cdiv(a.nout, tile), (unsigned)f->nch);
    hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds_bytes, st, a);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

// Which phase group each thread of the fast kernel owns.  A thread's LDS reads are at (round) M + c_g + j, c_g = (phi0-1 + g P M)
// div L: with groups in thread order, the 32 lanes of a ds_read_b32 group span ~32 P M / L addresses and collide two ways
// whenever that exceeds 32 (160//147: 1.88 LDS cycles per access instead of 1, 45 % of the kernel's LDS cycles measured as
// bank conflicts).  Any assignment of groups to lanes is legal (the taps live in registers, stores stay inside the same
// L-sample row), so the host picks, per 32-lane group, phase groups with distinct banks (greedy), keeps the identity when
// that is not better, and passes the table in the kernel arguments.
template <int P> void fir_lane_map(FirFastArgs& b) {
    const int NP = b.NP, nthreads = b.NP * b.RL;
    std::vector<int> c0(NP), ident(nthreads), greedy(nthreads);
    for (int g = 0; g < NP; ++g) c0[g] = (int)((b.phi0m1 + (int64_t)g * P * b.M) / b.L);
    const auto cycles = [&](const std::vector<int>& tab) {
        int total = 0;
        for (int w0 = 0; w0 < nthreads; w0 += 32) {
            int cnt[32] = {0}, addr[32][32];
            int worst = 1;
            for (int t = w0; t < std::min(w0 + 32, nthreads); ++t) {
                const int a = (t / NP) * b.M + c0[tab[t]], bank = a & 31;
                bool seen = false;
                for (int i = 0; i < cnt[bank]; ++i) seen = seen || addr[bank][i] == a;
                if (!seen) addr[bank][cnt[bank]++] = a;
                worst = std::max(worst, cnt[bank]);
            }
            total += worst;
        }
        return total;
    };
    std::vector<std::vector<char>> used(b.RL, std::vector<char>(NP, 0));
    for (int t = 0; t < nthreads; ++t) ident[t] = t % NP;
    for (int w0 = 0; w0 < nthreads; w0 += 32) {
        bool bank_used[32] = {false};
        for (int t = w0; t < std::min(w0 + 32, nthreads); ++t) {
            const int r = t / NP;
            int pick = -1, any = -1;
            for (int g = 0; g < NP && pick < 0; ++g) {
                if (used[r][g]) continue;
                if (any < 0) any = g;
                if (!bank_used[(r * b.M + c0[g]) & 31]) pick = g;
            }
            if (pick < 0) pick = any;
            used[r][pick] = 1;
            bank_used[(r * b.M + c0[pick]) & 31] = true;
            greedy[t] = pick;
        }
    }
    const std::vector<int>& best = cycles(greedy) < cycles(ident) && !MDSP_DBG(fir_identity_lanes) ? greedy : ident;
    for (int t = 0; t < 256; ++t) b.gmap[t] = (unsigned char)(t < nthreads ? best[t] : 0);
}

template <int TPC, int P> int fir_fast_launch(mdsp_fir_s* f, const FirArgs& a, hipStream_t st) {
    FirFastArgs b{};
    b.x = (const float*)a.x;
    b.hist = (const float*)a.hist;
    b.y = (float*)a.y;
    b.pfbT = (const float*)a.pfbT;
    b.xlen = a.xlen; b.ldx = a.ldx; b.ldy = a.ldy; b.nout = a.nout;
    b.phi0m1 = a.phi0m1; b.d0 = a.d0;
    b.L = a.L; b.M = a.M; b.tp = a.tp; b.hl = a.hl;
    b.nrounds = cdiv(a.nout, (int64_t)a.L);
    b.NP = (int)cdiv(a.L, P);
    b.RL = std::max(1, 256 / b.NP);
    fir_lane_map<P>(b);
    // rounds per tile: LDS budget ~48 KiB, at least RL rounds
    const int lds_kib = tunables().fir_lds_kib;
    int Q = (int)std::max<int64_t>(b.RL, ((int64_t)lds_kib * 1024 / 4 - a.M - (TPC + P)) / std::max(1, a.M));
    Q = std::min(Q, 512);
    Q = (int)std::min<int64_t>(Q, std::max<int64_t>(b.nrounds, 1));
    b.Q = Q;
    b.span = Q * a.M + a.M + TPC + P;
    const size_t lds_bytes = (size_t)b.span * sizeof(float);
    auto kern = polyphase_fast_kernel<TPC, P>;
    if (lds_bytes > 48 * 1024) MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const int64_t ntiles = cdiv(b.nrounds, (int64_t)Q);
    int wgs = P >= 4 ? 2 : (P == 3 ? 3 : 5);   // resident workgroups per CU (P = 2: 94 VGPRs x 4 waves, ~20 KiB LDS; 8 / 5 / 4 measured 2.64 / 2.59 / 2.67 ms on config 5; P = 4: 228 VGPRs)
    if (tunables().wg_per_cu > 0) wgs = tunables().wg_per_cu;
    const int64_t per = std::max<int64_t>(1, (int64_t)device_cu_count() * wgs / std::max<int64_t>(1, f->nch));
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, per), (unsigned)f->nch);
    hipLaunchKernelGGL(kern, grid, dim3(b.NP * b.RL), lds_bytes, st, b);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

// Fast path applies to Float32 taps x real Float32 signal with <= 64 taps per phase and <= 1024 phase groups.
bool mdsp::fir_fast_ok(const mdsp_fir_s* f, int P) {
    if (f->ctaps || f->acc_double || f->x_dtype != MDSP_F32 || f->tp > 64) return false;
    if (MDSP_DBG(fir_generic) || tunables().fir_exact || f->exact) return false;
    if (P >= 2 && (f->M > f->L || f->L < P)) return false;
    if (cdiv(f->L, P) > 256) return false;
    // the smallest tile fir_fast_launch stages is RL = 256 / NP rounds of M samples: a long decimation (1//200: 205 KiB) does not fit the LDS
    const int64_t RL = std::max<int64_t>(1, 256 / cdiv(f->L, (int64_t)P));
    return (RL * f->M + f->M + (f->tp + 7) / 8 * 8 + P) * (int64_t)sizeof(float) <= 150 * 1024;
}

namespace {

template <int P> int fir_fast_dispatch(mdsp_fir_s* f, const FirArgs& a, hipStream_t st) {
    const int tpc = (int)((f->tp + 7) / 8 * 8);
    switch (tpc) {
        case 8: return fir_fast_launch<8, P>(f, a, st);
        case 16: return fir_fast_launch<16, P>(f, a, st);
        case 24: return fir_fast_launch<24, P>(f, a, st);
        case 32: return fir_fast_launch<32, P>(f, a, st);
        case 40: return fir_fast_launch<40, P>(f, a, st);
        case 48: return fir_fast_launch<48, P>(f, a, st);
        case 56: return fir_fast_launch<56, P>(f, a, st);
        default: return fir_fast_launch<64, P>(f, a, st);
    }
}

// A filter whose shape has a line in the box's choice file (common.h FirChoice) is dispatched under that line's knob values: the calling thread's view of
// the tunables for the duration of the scope.
struct FirChoiceScope {
    Tunables t;
    const Tunables* prev = nullptr;
    bool on = false;
    explicit FirChoiceScope(const mdsp_fir_s* f) {
        const Tunables& base = tunables();
        if (base.fir_choices.empty()) return;   // (the usual case: no choice file named)
        for (const FirChoice& c : base.fir_choices) {
            if (c.L != f->L || c.M != f->M || c.hlen != f->hlen || c.taps_dtype != f->taps_dtype || c.x_dtype != f->x_dtype) continue;
            t = base;
            t.fir_choices.clear();   // the view carries the knob values only
            for (int i = 0; i < c.nset; ++i)
                if (int* field = fir_choice_field(t, c.field[i])) *field = c.value[i];
            prev = tunables_override(&t);
            on = true;
            break;
        }
    }
    ~FirChoiceScope() {
        if (on) tunables_override(prev);
    }
    FirChoiceScope(const FirChoiceScope&) = delete;
    FirChoiceScope& operator=(const FirChoiceScope&) = delete;
};

bool fir_reg_use(const mdsp_fir_s* f) {
    if (MDSP_DBG(fir_generic) || tunables().fir_exact || f->exact || f->kind == 4) return false;
    if (f->ctaps) return fir_creg_ok(f->x_dtype, f->acc_double, f->tp, f->L, f->M);
    return fir_reg_ok(f->x_dtype, f->acc_double, f->tp, f->L, f->M);
}

// what the register-tap units (fir_reg.hip, fir_creg.hip) take from a launch's arguments; their run functions fill in the geometry
FirRegArgs fir_reg_args(const FirArgs& a) {
    FirRegArgs b{};
    b.x = a.x; b.hist = a.hist; b.y = a.y; b.pfbT = a.pfbT;
    b.xlen = a.xlen; b.ldx = a.ldx; b.ldy = a.ldy; b.nout = a.nout;
    b.phi0m1 = a.phi0m1; b.d0 = a.d0;
    b.L = a.L; b.M = a.M; b.tp = a.tp; b.hl = a.hl;
    return b;
}

// complex taps: the complex register-tap kernel where its predicate claims the shape, the generic kernel with H = cx<R> everywhere else
int fir_dispatch_ctaps(mdsp_fir_s* f, FirArgs& a, hipStream_t st) {
    if (fir_reg_use(f)) {
        FirRegArgs b = fir_reg_args(a);
        return fir_creg_run(f->x_dtype, f->acc_double, b, f->nch, st);
    }
    const bool d = f->acc_double;
    switch (f->x_dtype) {
        case MDSP_F32: return d ? fir_launch<float, cx<double>, double, double, cx<double>>(f, a, st) : fir_launch<float, cx<float>, float, float, cx<float>>(f, a, st);
        case MDSP_F64: return fir_launch<double, cx<double>, double, double, cx<double>>(f, a, st);
        case MDSP_C32: return d ? fir_launch<cx<float>, cx<double>, double, cx<double>, cx<double>>(f, a, st) : fir_launch<cx<float>, cx<float>, float, cx<float>, cx<float>>(f, a, st);
        default: return fir_launch<cx<double>, cx<double>, double, cx<double>, cx<double>>(f, a, st);
    }
}

int fir_dispatch(mdsp_fir_s* f, FirArgs& a, hipStream_t st) {
    const FirChoiceScope choice(f);
    if (f->ctaps) return fir_dispatch_ctaps(f, a, st);
    {
        const DecGeo dg = fir_dec_geo(f);
        if (dg.ok) return fir_dec_dispatch(f, a, dg, st);
    }
    if (fir_mm_use(f, a)) return fir_mm_dispatch(f, a, st);
    if (tunables().fir_p == 4 && f->tp <= 32 && fir_fast_ok(f, 4)) return fir_fast_dispatch<4>(f, a, st);   // tuning: four residues per thread
    if (tunables().fir_p == 3 && f->tp <= 32 && fir_fast_ok(f, 3)) return fir_fast_dispatch<3>(f, a, st);   // tuning: three residues per thread
    if (fir_fast_ok(f, 2)) return fir_fast_dispatch<2>(f, a, st);
    if (fir_fast_ok(f, 1)) return fir_fast_dispatch<1>(f, a, st);
    if (fir_reg_use(f)) {   // round 6: register taps for every other signal type where the matrix-core tile missed the LDS (fir_reg.hip)
        FirRegArgs b = fir_reg_args(a);
        return fir_reg_run(f->x_dtype, f->acc_double, b, f->nch, st);
    }
    const bool d = f->acc_double;
    switch (f->x_dtype) {
        case MDSP_F32: return d ? fir_launch<float, double, double>(f, a, st) : fir_launch<float, float, float>(f, a, st);
        case MDSP_F64: return fir_launch<double, double, double>(f, a, st);
        case MDSP_C32: return d ? fir_launch<cx<float>, cx<double>, double>(f, a, st) : fir_launch<cx<float>, cx<float>, float>(f, a, st);
        default: return fir_launch<cx<double>, cx<double>, double>(f, a, st);
    }
}

template <typename XS> int shiftin_launch(mdsp_fir_s* f, const void* x, int64_t xlen, int64_t ldx, hipStream_t st) {
    if (f->hl == 0) return MDSP_OK;
    const int nxt = f->cur ^ 1;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(f->hl, 256), 64), (unsigned)f->nch);
    hipLaunchKernelGGL(shiftin_kernel<XS>, grid, dim3(256), 0, st, (const XS*)x, f->hist[f->cur].as<XS>(), f->hist[nxt].as<XS>(), xlen, ldx, (int)f->hl);
    MDSP_LAUNCH_CHECK();
    f->cur = nxt;
    return MDSP_OK;
}

}  // namespace

int mdsp::shiftin_dispatch(mdsp_fir_s* f, const void* x, int64_t xlen, int64_t ldx, hipStream_t st) {
    if (xlen == 0) return MDSP_OK;
    switch (f->x_dtype) {
        case MDSP_F32: return shiftin_launch<float>(f, x, xlen, ldx, st);
        case MDSP_F64: return shiftin_launch<double>(f, x, xlen, ldx, st);
        case MDSP_C32: return shiftin_launch<cx<float>>(f, x, xlen, ldx, st);
        default: return shiftin_launch<cx<double>>(f, x, xlen, ldx, st);
    }
}

int mdsp::fir_reset_on(mdsp_fir_s* f, hipStream_t st, bool async) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    const size_t hbytes = dtype_size(f->x_dtype) * (size_t)std::max<int64_t>(1, f->hl) * (size_t)f->nch;
    if (async) MDSP_HIP(hipMemsetAsync(f->hist[f->cur].p, 0, hbytes, st));   // stream-ordered: the caller's next exec runs on the same stream
    else MDSP_HIP(hipMemset(f->hist[f->cur].p, 0, hbytes));
    f->phi_idx = 1;
    f->input_deficit = 1;
    return MDSP_OK;
}

extern "C" {

int mdsp_fir_create(mdsp_fir* fo, const void* taps_host, int64_t hlen, int64_t L, int64_t M, int taps_dtype, int x_dtype, int64_t nch) {
    if (!fo) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle pointer is NULL");
    *fo = nullptr;
    if (!taps_host || hlen < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter taps must be non-empty");
    if (L < 1 || M < 1) MDSP_FAIL(MDSP_ERR_DOMAIN, "resampling ratio must be positive");
    if (!dtype_valid(taps_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid taps dtype");
    if (!dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid x dtype");
    if (nch < 1 || nch > 65535) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nch must be in [1, 65535]");
    const int64_t g = gcd64(L, M);  // Rational normalisation (numerator / denominator of L//M)
    L /= g;
    M /= g;
    if (L > (int64_t(1) << 20) || M > (int64_t(1) << 30)) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "ratio terms too large");
    auto f = new mdsp_fir_s();
    f->L = L;
    f->M = M;
    f->hlen = hlen;
    f->nch = nch;
    f->taps_dtype = taps_dtype;
    f->x_dtype = x_dtype;
    f->kind = (L == 1 && M == 1) ? 0 : (M == 1 ? 1 : (L == 1 ? 2 : 3));
    f->tp = cdiv(hlen, L);                       // taps2pfb: tapsPerPhase = ceil(hLen / Nphi)   (stream_filt.jl:296)
    f->hl = f->tp - 1;                           // historyLen (:163,:166,:169,:172)
    f->ctaps = dtype_is_complex(taps_dtype);
    f->acc_double = dtype_is_double(taps_dtype) || dtype_is_double(x_dtype);  // promote_type(Th, Tx)
    f->out_dtype = (f->ctaps || dtype_is_complex(x_dtype)) ? (f->acc_double ? MDSP_C64 : MDSP_C32) : (f->acc_double ? MDSP_F64 : MDSP_F32);
    // pfbT[i*L + c] = pfb[i+1, c+1] with pfb[row, col] = h[(tp-row)*L + col] (1-based rows from the bottom, :300-304); complex taps: (re, im) pairs
    const size_t nc = f->ctaps ? 2 : 1, np = (size_t)(f->tp * L) * nc;
    const bool taps_f32 = !dtype_is_double(taps_dtype);
    std::vector<double> pd(np, 0.0);
    for (int64_t row = 0; row < f->tp; ++row)       // row 0 = top of the matrix
        for (int64_t col = 0; col < L; ++col) {
            const int64_t hidx = (f->tp - 1 - row) * L + col;  // bottom row holds h[0..L)
            if (hidx >= hlen) continue;
            for (size_t c = 0; c < nc; ++c) {
                const size_t src = (size_t)hidx * nc + c;
                pd[(size_t)(row * L + col) * nc + c] = taps_f32 ? (double)((const float*)taps_host)[src] : ((const double*)taps_host)[src];
            }
        }
    int st = MDSP_OK;
    if (f->acc_double) {
        st = f->pfbT.reserve(sizeof(double) * np);
        if (st == MDSP_OK && hipMemcpy(f->pfbT.p, pd.data(), sizeof(double) * np, hipMemcpyHostToDevice) != hipSuccess) st = set_error(MDSP_ERR_DEVICE, "tap upload failed");
    } else {
        std::vector<float> pf(np);
        for (size_t i = 0; i < np; ++i) pf[i] = (float)pd[i];
        st = f->pfbT.reserve(sizeof(float) * np);
        if (st == MDSP_OK && hipMemcpy(f->pfbT.p, pf.data(), sizeof(float) * np, hipMemcpyHostToDevice) != hipSuccess) st = set_error(MDSP_ERR_DEVICE, "tap upload failed");
    }
    const size_t hbytes = dtype_size(x_dtype) * (size_t)std::max<int64_t>(1, f->hl) * (size_t)nch;
    for (int b = 0; b < 2 && st == MDSP_OK; ++b) {
        st = f->hist[b].reserve(hbytes);
        if (st == MDSP_OK && hipMemset(f->hist[b].p, 0, hbytes) != hipSuccess) st = set_error(MDSP_ERR_DEVICE, "history init failed");
    }
    if (st != MDSP_OK) {
        delete f;
        return st;
    }
    *fo = f;
    return MDSP_OK;
}

int mdsp_fir_destroy(mdsp_fir f) {
    delete f;
    return MDSP_OK;
}

int mdsp_fir_set_exact(mdsp_fir f, int exact) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    f->exact = exact != 0;
    return MDSP_OK;
}

int mdsp_fir_reset(mdsp_fir f) { return fir_reset_on(f, nullptr, false); }

int mdsp_fir_setphase(mdsp_fir f, double phi) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (!(phi >= 0)) MDSP_FAIL(MDSP_ERR_DOMAIN, "phi must be >= 0");
    if (f->kind == 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "setphase! is not defined for a single-rate FIRFilter");
    if (f->kind == 2) {  // :216-221
        f->input_deficit += round_half_even(phi);
    } else {  // :223-229
        const int64_t q = round_half_even(phi * (double)f->L);
        f->input_deficit += q / f->L;
        f->phi_idx = q % f->L + 1;
    }
    return MDSP_OK;
}

int mdsp_fir_timedelay(mdsp_fir f, double* tau) {
    if (!f || !tau) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    *tau = (f->kind == 1 || f->kind == 3) ? (double)(f->hlen - 1) / (double)(2 * f->L) : (double)(f->hlen - 1) / 2.0;
    return MDSP_OK;
}

int mdsp_fir_outputlength(mdsp_fir f, int64_t inputlength, int64_t* outlen) {
    if (!f || !outlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    if (f->kind == 0) *outlen = inputlength;
    else *outlen = mdsp_outputlength(inputlength - f->input_deficit + 1, f->L, f->M, f->kind == 2 ? 1 : f->phi_idx);
    return MDSP_OK;
}

int mdsp_fir_inputlength(mdsp_fir f, int64_t outputlength, int round_up, int64_t* inlen) {
    if (!f || !inlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    if (f->kind == 0) *inlen = outputlength;
    else *inlen = mdsp_inputlength(outputlength, f->L, f->M, f->kind == 2 ? 1 : f->phi_idx, round_up) + f->input_deficit - 1;
    return MDSP_OK;
}

int mdsp_fir_info(mdsp_fir f, int* kind, int64_t* L, int64_t* M, int64_t* taps_per_phase, int64_t* history_len, int* out_dtype) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (kind) *kind = f->kind;
    if (L) *L = f->L;
    if (M) *M = f->M;
    if (taps_per_phase) *taps_per_phase = f->tp;
    if (history_len) *history_len = f->hl;
    if (out_dtype) *out_dtype = f->out_dtype;
    return MDSP_OK;
}

int mdsp_fir_mm_geometry(int64_t L, int64_t M, int64_t hlen, int taps_dtype, int x_dtype, int64_t* out12) {
    if (!out12) MDSP_FAIL(MDSP_ERR_ARGUMENT, "out is NULL");
    if (L < 1 || M < 1 || hlen < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "L, M, hlen must be positive");
    if (!dtype_valid(taps_dtype) || !dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    const int64_t g0 = gcd64(L, M);
    mdsp_fir_s f;   // no device objects are touched: pure geometry
    f.L = L / g0;
    f.M = M / g0;
    f.hlen = hlen;
    f.tp = cdiv(hlen, f.L);
    f.hl = f.tp - 1;
    f.taps_dtype = taps_dtype;
    f.x_dtype = x_dtype;
    f.ctaps = dtype_is_complex(taps_dtype);   // (fits = 0: the matrix-core kernel takes real taps only)
    f.acc_double = dtype_is_double(taps_dtype) || dtype_is_double(x_dtype);
    const FirChoiceScope choice(&f);
    const FirMGeo g = fir_mm_geo(&f);
    const int64_t v[12] = {g.ok ? 1 : 0, g.RB, g.Lr, g.Mr, g.NB, g.NG, g.steps, g.CH, g.CS, g.nd, g.ns, (int64_t)g.lds_bytes};
    for (int i = 0; i < 12; ++i) out12[i] = v[i];
    return MDSP_OK;
}

int mdsp_fir_kernel_path(mdsp_fir f, int64_t xlen, int* path) {
    if (!f || !path) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    if (xlen < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    const int64_t phi0 = f->kind == 2 ? 1 : f->phi_idx;
    const int64_t d0 = f->kind == 0 ? 1 : f->input_deficit;
    FirArgs a{};
    a.nout = f->kind == 0 ? xlen : (xlen < d0 ? 0 : mdsp_outputlength(xlen - d0 + 1, f->L, f->M, phi0));
    a.L = (int)f->L;
    a.M = (int)f->M;
    const FirChoiceScope choice(f);
    if (f->ctaps) *path = fir_reg_use(f) ? 1 : 0;   // complex taps: 1 the complex register-tap kernel (fir_creg.hip), 0 generic
    else *path = fir_dec_geo(f).ok ? 3 : fir_mm_use(f, a) ? 2 : (fir_fast_ok(f, 2) || fir_fast_ok(f, 1) || fir_reg_use(f)) ? 1 : 0;   // 3: decimator kernel, 2: matrix cores, 1: register taps, 0: generic
    return MDSP_OK;
}

int mdsp_fir_get_state(mdsp_fir f, int64_t* phi_idx, int64_t* input_deficit, void* history_host) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (phi_idx) *phi_idx = f->phi_idx;
    if (input_deficit) *input_deficit = f->input_deficit;
    if (history_host && f->hl > 0) {
        MDSP_HIP(hipDeviceSynchronize());
        MDSP_HIP(hipMemcpy(history_host, f->hist[f->cur].p, dtype_size(f->x_dtype) * (size_t)f->hl * (size_t)f->nch, hipMemcpyDeviceToHost));
    }
    return MDSP_OK;
}

int mdsp_fir_set_state(mdsp_fir f, int64_t phi_idx, int64_t input_deficit, const void* history_host) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (phi_idx < 1 || phi_idx > f->L || input_deficit < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "state out of range");
    f->phi_idx = phi_idx;
    f->input_deficit = input_deficit;
    if (history_host && f->hl > 0) {
        MDSP_HIP(hipDeviceSynchronize());
        MDSP_HIP(hipMemcpy(f->hist[f->cur].p, history_host, dtype_size(f->x_dtype) * (size_t)f->hl * (size_t)f->nch, hipMemcpyHostToDevice));
    }
    return MDSP_OK;
}

int mdsp_fir_exec(mdsp_fir f, const void* x_dev, int64_t xlen, int64_t ldx, void* y_dev, int64_t ycap, int64_t ldy, int64_t* nwritten,
                  void* stream) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (xlen < 0 || ycap < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (f->nch > 1 && ldx < xlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldx smaller than xlen");
    hipStream_t st = as_stream(stream);
    if (nwritten) *nwritten = 0;
    if (f->kind != 0 && xlen < f->input_deficit) {  // stream_filt.jl:483-487 (and :443-447, :529-533)
        MDSP_TRY(shiftin_dispatch(f, x_dev, xlen, ldx, st));
        f->input_deficit -= xlen;
        return MDSP_OK;
    }
    const int64_t phi0 = f->kind == 2 ? 1 : f->phi_idx;
    const int64_t d0 = f->kind == 0 ? 1 : f->input_deficit;
    const int64_t nout = f->kind == 0 ? xlen : mdsp_outputlength(xlen - d0 + 1, f->L, f->M, phi0);
    if (ycap < nout) MDSP_FAIL(MDSP_ERR_ARGUMENT, "buffer is too small: need %lld, have %lld", (long long)nout, (long long)ycap);
    if (f->nch > 1 && ldy < nout) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldy smaller than the output length");
    if (nout > 0) {
        if (!x_dev || !y_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
        FirArgs a{};
        a.x = x_dev;
        a.hist = f->hist[f->cur].p;
        a.y = y_dev;
        a.pfbT = f->pfbT.p;
        a.xlen = xlen;
        a.ldx = ldx;
        a.ldy = ldy;
        a.nout = nout;
        a.phi0m1 = phi0 - 1;
        a.d0 = d0;
        a.L = (int)f->L;
        a.M = (int)f->M;
        a.tp = (int)f->tp;
        a.hl = (int)f->hl;
        MDSP_TRY(fir_dispatch(f, a, st));
    }
    // state advance: closed form of the loop's final (inputIdx, phiIdx)   (:506-511)
    const __int128 p_end = (__int128)(phi0 - 1) + (__int128)nout * f->M;
    const int64_t input_idx_end = d0 + (int64_t)(p_end / f->L);
    if (f->kind == 1 || f->kind == 3) f->phi_idx = (int64_t)(p_end % f->L) + 1;
    if (f->kind == 1) f->input_deficit = 1;                              // :465
    else if (f->kind != 0) f->input_deficit = input_idx_end - xlen;      // :511, :554
    MDSP_TRY(shiftin_dispatch(f, x_dev, xlen, ldx, st));                 // :512
    if (nwritten) *nwritten = nout;
    return MDSP_OK;
}

// filt(::FIRFilter, x) / resample(x, ratio, h) of host arrays (stream_filt.jl:627-637, :688-775): the stream goes through the filter in time
// chunks of all channels -- exactly the reference's streaming use of a FIRFilter, whose state (phase index, input deficit, history) the object
// carries from chunk to chunk, so the chunked result is the one-shot result bit for bit and the filter ends in the same state.
int mdsp_fir_exec_host(mdsp_fir f, const void* x_host, int64_t xlen, int64_t ldx, void* y_host, int64_t ycap, int64_t ldy, int64_t* nwritten,
                       int flags) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (xlen < 0 || ycap < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (f->nch > 1 && ldx < xlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldx smaller than xlen");
    if (nwritten) *nwritten = 0;
    int64_t total = 0;
    MDSP_TRY(mdsp_fir_outputlength(f, xlen, &total));
    if (ycap < total) MDSP_FAIL(MDSP_ERR_ARGUMENT, "buffer is too small: need %lld, have %lld", (long long)total, (long long)ycap);
    if (f->nch > 1 && ldy < total) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldy smaller than the output length");
    if (xlen == 0) return MDSP_OK;
    if (!x_host || (total > 0 && !y_host)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const bool pinned = (flags & MDSP_HOST_PINNED) != 0;
    const size_t esz = dtype_size(f->x_dtype), osz = dtype_size(f->out_dtype);
    const int64_t nch = f->nch;
    // samples per channel and chunk: ~host_chunk_mib of input and output together
    const double per_sample = (double)esz + (double)osz * (double)f->L / (double)f->M;
    const int64_t cl_max = std::max<int64_t>(4096, (int64_t)((double)((int64_t)tunables().host_chunk_mib << 20) / per_sample / (double)nch));
    const int64_t ocap = (int64_t)(((__int128)cl_max * f->L) / f->M) + 2;      // outputs of a chunk never exceed ceil(cl L / M) + 1
    hostpipe::Session ss((size_t)cl_max * (size_t)nch * esz, (size_t)ocap * (size_t)nch * osz, pinned);
    int rc = ss.status();
    int64_t done = 0;
    for (int64_t x0 = 0; x0 < xlen && rc == MDSP_OK; x0 += cl_max) {
        hostpipe::Lane* ln = nullptr;
        if ((rc = ss.acquire(&ln)) != MDSP_OK) break;
        const int64_t cl = std::min(cl_max, xlen - x0);
        if ((rc = ss.upload(ln, static_cast<const char*>(x_host) + (size_t)x0 * esz, (size_t)ldx * esz, (size_t)cl * esz, (size_t)nch)) != MDSP_OK) break;
        int64_t nw = 0;
        if ((rc = mdsp_fir_exec(f, ln->din.p, cl, cl, ln->dout.p, ocap, ocap, &nw, ss.kstream())) != MDSP_OK) break;
        rc = ss.download(ln, static_cast<char*>(y_host) + (size_t)done * osz, (size_t)ldy * osz, (size_t)nw * osz, (size_t)nch, 0, (size_t)ocap * osz);
        done += nw;
    }
    rc = ss.finish(rc);
    if (rc == MDSP_OK && done != total) rc = set_error(MDSP_ERR_ASSERTION, "chunked filtering wrote %lld outputs, the closed form says %lld", (long long)done, (long long)total);
    if (nwritten) *nwritten = done;
    return rc;
}

}  // extern "C"
