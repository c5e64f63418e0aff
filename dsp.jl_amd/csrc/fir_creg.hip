// Register-tap polyphase kernel for complex taps (fir_creg.h).  The reference loop it replaces: Filters/stream_filt.jl:496-509 (FIRRational filt!) with
// the generic unsafe_dot of util.jl:225-283 -- one dot product of tapsPerPhi complex taps per output, oldest sample first, no conjugation.
//
// Same structure as fir_reg.hip: outputs m = q L + s all use phase phi_s and the window that starts at q M + c_s, so a thread owns P consecutive
// residues for the whole launch, keeps their taps -- (re, im) pairs, pre-shifted by delta_k = c_{s+k} - c_s -- in registers, and per round reads ONE
// window of TPC + P - 1 staged samples from LDS for its P outputs.  The signal is staged in its own class (Z = R for a real signal, cx<R> for a complex
// one; R the arithmetic precision), through buffer-descriptor loads with zero fill past the end.
//   complex taps x real signal:     (acc.re, acc.im) += (h.re, h.im) x                 one packed multiply-add per tap in Float32
//   complex taps x complex signal:  acc += h.re (x.re, x.im); acc += h.im (-x.im, x.re)  two packed multiply-adds per tap in Float32, four v_fma_f64 in Float64
// Zero taps in front of / behind a phase add exact zeros, so results are those of the generic kernel's chain for finite samples; a non-finite sample inside
// the P - 1 extra window positions widens the reference's hole, which is what mdsp_fir_set_exact is for.
#include "fir_creg.h"

#include "devio.h"
#include "fir_op.h"

using namespace mdsp;
using mdsp::firop::to_acc;
using mdsp::fft::cx;

namespace {

template <typename R> using v2 = R __attribute__((ext_vector_type(2)));

// acc += h x, h = (re, im)
template <typename R> __device__ __forceinline__ void cfma(v2<R>& acc, v2<R> h, R x) { acc = __builtin_elementwise_fma(v2<R>{x, x}, h, acc); }
template <typename R> __device__ __forceinline__ void cfma(v2<R>& acc, v2<R> h, cx<R> x) {
    acc = __builtin_elementwise_fma(v2<R>{h.x, h.x}, v2<R>{x.x, x.y}, acc);
    acc = __builtin_elementwise_fma(v2<R>{h.y, h.y}, v2<R>{-x.y, x.x}, acc);
}
// Float32: the same two multiply-adds as v_pk_fma_f32 with the broadcast, swap and sign in the operand modifiers.  Written as assembly because the
// compiler otherwise keeps (h.re, h.re) and (h.im, h.im) as separate register pairs -- twice the tap registers -- and builds (-x.im, x.re) with a
// v_xor and a v_mov per sample.
__device__ __forceinline__ void cfma(v2<float>& acc, v2<float> h, cx<float> x) {
    const v2<float> xv = {x.x, x.y};
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(h), "v"(xv));                  // acc += h.re (x.re, x.im)
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "+v"(acc) : "v"(h), "v"(xv));   // acc += h.im (-x.im, x.re)
}
// Float32, real signal: two consecutive samples sit in one register pair and the multiply-add picks its sample by op_sel -- the compiler's own form keeps a
// broadcast pair (x, x) per sample in registers (262 registers at 2 x 41 taps: one wave per SIMD instead of two).  HI: the pair's second sample.
template <bool HI> __device__ __forceinline__ void cfma_pair(v2<float>& acc, v2<float> h, v2<float> xx) {
    if constexpr (HI) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(h), "v"(xx));   // acc += (h.re, h.im) xx.hi
    else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(h), "v"(xx));               // acc += (h.re, h.im) xx.lo
}

// XS: storage type of x; Z: staged type (R or cx<R>); R: arithmetic precision.  Output / accumulator / tap type: cx<R>.
template <typename XS, typename Z, typename R, int TPC, int P, int LB>
__global__ __launch_bounds__(LB) void polyphase_creg_kernel(FirRegArgs a) {
    constexpr int W = TPC + P - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char creg_smem[];
    Z* zs = reinterpret_cast<Z*>(creg_smem);
    const int64_t ch = blockIdx.y;
    const int g = threadIdx.x % a.NP, r = threadIdx.x / a.NP;
    const XS* xc = static_cast<const XS*>(a.x) + ch * a.ldx;
    const XS* hc = static_cast<const XS*>(a.hist) + ch * (int64_t)a.hl;
    cx<R>* yc = static_cast<cx<R>*>(a.y) + ch * a.ldy;
    const cx<R>* pfb = static_cast<const cx<R>*>(a.pfbT);
    // per-thread constants: the window offset of residue 0 of the group, the taps of its P residues shifted to that window
    const int s0 = g * P;
    bool valid[P];
    v2<R> h[P][W];
    const int64_t cbase = a.d0 - 1;   // c_s = cbase + (phi0m1 + s M) div L
    int c0rel = 0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int s = s0 + k;
        valid[k] = s < a.L;
        const int64_t p = a.phi0m1 + (int64_t)(valid[k] ? s : 0) * a.M;
        const int phi = (int)(p % a.L);
        const int crel = (int)(p / a.L);
        if (k == 0) c0rel = crel;
        const int delta = valid[k] ? crel - c0rel : 0;   // 0 .. P - 1 (M <= L whenever P > 1)
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int i = j - delta;
            cx<R> t{};
            if (valid[k] && i >= 0 && i < a.tp) t = pfb[(int64_t)i * a.L + phi];
            h[k][j] = v2<R>{t.x, t.y};
        }
    }
    const int64_t ntiles = (a.nrounds + a.Q - 1) / a.Q;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t q0 = tile * a.Q;
        const int nq = (int)std::min<int64_t>(a.Q, a.nrounds - q0);
        const int64_t z0 = q0 * a.M + cbase;          // first staged index into [history ; x]
        const int nz = nq * a.M + a.M + W;            // <= span = Q M + M + W samples of LDS
        __syncthreads();   // the previous tile is consumed
        if (z0 >= a.hl) {  // steady state: the tile lies inside x (descriptor re-based at the tile start: zeros past the end of the signal)
            const XS* src = xc + (z0 - a.hl);
            const __amdgpu_buffer_rsrc_t rs = io::make_rsrc(src, (a.xlen - (z0 - a.hl)) * (int64_t)sizeof(XS));
            const int step = blockDim.x;
            for (int k2 = threadIdx.x; k2 < nz; k2 += 4 * step) {
                XS v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = io::Ld<XS>::load(rs, (k2 + u * step) * (int)sizeof(XS));
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k2 + u * step < nz) zs[k2 + u * step] = to_acc(v[u], (Z*)nullptr);
            }
        } else {           // the first tile(s) straddle the history
            for (int k2 = threadIdx.x; k2 < nz; k2 += blockDim.x) {
                const int64_t zi = z0 + k2;
                Z v{};
                if (zi < a.hl) v = to_acc(hc[zi], (Z*)nullptr);
                else if (zi - a.hl < a.xlen) v = to_acc(xc[zi - a.hl], (Z*)nullptr);
                zs[k2] = v;
            }
        }
        __syncthreads();
        if (valid[0]) {
            for (int q = r; q < nq; q += a.RL) {
                const Z* zp = zs + q * a.M + c0rel;
                v2<R> acc[P];
#pragma unroll
                for (int k = 0; k < P; ++k) acc[k] = v2<R>{(R)0, (R)0};
                if constexpr (sizeof(Z) == 4) {   // Float32 real signal: samples two at a time (same order per chain: j, then j + 1)
#pragma unroll
                    for (int j = 0; j < W; j += 2) {
                        const v2<float> xx = {zp[j], j + 1 < W ? zp[j + 1] : 0.0f};
#pragma unroll
                        for (int k = 0; k < P; ++k) {
                            cfma_pair<false>(acc[k], h[k][j], xx);
                            if (j + 1 < W) cfma_pair<true>(acc[k], h[k][j + 1], xx);
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const Z xv = zp[j];
#pragma unroll
                        for (int k = 0; k < P; ++k) cfma(acc[k], h[k][j], xv);
                    }
                }
                const int64_t m = (q0 + q) * a.L + s0;
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (valid[k] && m + k < a.nout) yc[m + k] = cx<R>{acc[k].x, acc[k].y};
            }
        }
    }
}

// Taps per phase rounded up to the next instantiated window: steps of 8 as fir_reg.hip's tpc_of, up to what the register budget admits at all
// (Float32, one residue per thread: 112 pairs = 224 registers).
int ctpc_of(int64_t tp) { return tp <= 64 ? (int)((tp + 7) / 8 * 8) : tp <= 80 ? 80 : tp <= 96 ? 96 : tp <= 112 ? 112 : 0; }
// Registers of the taps: P (TPC + P - 1) complex values of R, against 230 at <= 256 threads (one wave per SIMD, 512 registers: the window in flight takes
// as many as the taps) and 96 at up to 1024 threads (128 registers) -- fir_reg.hip's budgets.  A ComplexF64 staged sample is four registers feeding four
// v_fma_f64 on aligned pairs, and there the compiler spills earlier (ComplexF64 window, 2 x 25 taps: 376 bytes of scratch; 1024 threads, 16 taps: 152):
// those two budgets are 170 and 48.  Every instantiation below compiles without scratch (launch() asserts it).  Largest TPC per case:
//                                       P = 1, <= 256 groups   P = 2, <= 256 groups   P = 1, <= 1024 groups
//   Float32 arithmetic                         112                     56                     48
//   Float64 arithmetic, real signal             56                     24                     24
//   Float64 arithmetic, complex signal          56                     16                      8
// zc: parts per staged sample (1 real signal, 2 complex)
constexpr bool cfits(int tpc, int P, int rbytes, bool wide, int zc) {
    const bool c64 = rbytes == 8 && zc == 2;
    return P * (tpc + P - 1) * 2 * (rbytes / 4) <= (wide ? (c64 ? 48 : 96) : (P == 2 && c64 ? 170 : 230));
}
// the largest tile launch() stages: Q = RL rounds of M samples plus the window, within the 150 KiB of LDS
bool clds_fits(int tpc, int P, int zbytes, int64_t L, int64_t M) {
    const int64_t NP = cdiv(L, (int64_t)P), RL = NP <= 256 ? std::max<int64_t>(1, 256 / NP) : 1;
    return (RL * M + M + tpc + P - 1) * zbytes <= 150 * 1024;
}
// residues per thread: 2 where both the pair's taps and its <= 256 phase groups fit, else 1 (<= 256 groups, or <= 1024 with the smaller budget), else 0
int cchoose_p(int x_dtype, bool acc_double, int64_t tp, int64_t L, int64_t M) {
    const int tpc = ctpc_of(tp), rbytes = acc_double ? 8 : 4, zc = dtype_is_complex(x_dtype) ? 2 : 1, zbytes = rbytes * zc;
    if (tpc == 0 || L > 1024) return 0;
    if (M <= L && L >= 2 && cdiv(L, (int64_t)2) <= 256 && cfits(tpc, 2, rbytes, false, zc) && clds_fits(tpc, 2, zbytes, L, M)) return 2;
    if (cfits(tpc, 1, rbytes, L > 256, zc) && clds_fits(tpc, 1, zbytes, L, M)) return 1;
    return 0;
}

template <typename XS, typename Z, typename R, int TPC, int P> int launch(FirRegArgs& a, int64_t nch, hipStream_t st) {
    a.NP = (int)cdiv(a.L, P);
    constexpr int W = TPC + P - 1;
    const bool small = a.NP <= 256;
    a.RL = small ? std::max(1, 256 / a.NP) : 1;
    // rounds per tile: ~48 KiB of staged samples, at least RL rounds
    const int64_t budget = (int64_t)48 * 1024 / (int64_t)sizeof(Z);
    int Q = (int)std::max<int64_t>(a.RL, (budget - a.M - W) / std::max(1, a.M));
    Q = std::min(Q, 512);
    Q = (int)std::min<int64_t>(Q, std::max<int64_t>(a.nrounds, 1));
    a.Q = Q;
    a.span = Q * a.M + a.M + W;
    const size_t lds_bytes = (size_t)a.span * sizeof(Z);
    if (lds_bytes > 150 * 1024) MDSP_FAIL(MDSP_ERR_ASSERTION, "complex register-tap polyphase kernel: tile of %zu bytes (M=%d)", lds_bytes, a.M);   // (clds_fits)
    const int64_t ntiles = cdiv(a.nrounds, (int64_t)Q);
    // resident workgroups per CU: what the kernel's registers and the tile's LDS admit together (fir_reg.hip)
    auto go = [&](auto kern) -> int {
        hipFuncAttributes fa{};
        MDSP_HIP(hipFuncGetAttributes(&fa, (const void*)kern));
        if (fa.localSizeBytes != 0) MDSP_FAIL(MDSP_ERR_ASSERTION, "complex register-tap polyphase kernel (%d taps, %d residues): %zu bytes of scratch", TPC, P, (size_t)fa.localSizeBytes);
        const int regs = std::max(8, (fa.numRegs + 7) / 8 * 8), waves = (a.NP * a.RL + 63) / 64;
        const int by_regs = std::max(1, std::min(8, 512 / regs) * 4 / waves), by_lds = (int)std::max<size_t>(1, (size_t)(150 * 1024) / lds_bytes);
        const int wgs = tunables().wg_per_cu > 0 ? tunables().wg_per_cu : std::min({4, by_regs, by_lds});
        const int64_t per = std::max<int64_t>(1, (int64_t)device_cu_count() * wgs / std::max<int64_t>(1, nch));
        const dim3 grid((unsigned)std::min<int64_t>(ntiles, per), (unsigned)nch);
        if (lds_bytes > 48 * 1024) MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(kern, grid, dim3(a.NP * a.RL), lds_bytes, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    };
    constexpr int ZC = (int)(sizeof(Z) / sizeof(R));
    if (small) {
        if constexpr (cfits(TPC, P, (int)sizeof(R), false, ZC)) return go(polyphase_creg_kernel<XS, Z, R, TPC, P, 256>);
    } else {
        if constexpr (P == 1 && cfits(TPC, 1, (int)sizeof(R), true, ZC)) return go(polyphase_creg_kernel<XS, Z, R, TPC, P, 1024>);
    }
    MDSP_FAIL(MDSP_ERR_ASSERTION, "complex register-tap polyphase kernel: %d phase groups of %d taps are not instantiated", a.NP, TPC);
}

// only the (TPC, P) pairs cfits() admits are instantiated: launch<> of any other pair holds no kernel
template <typename XS, typename Z, typename R, int P> int dispatch_tpc(FirRegArgs& a, int64_t nch, hipStream_t st) {
    switch (ctpc_of(a.tp)) {
#define MDSP_CREG_CASE(T)                                                                                       \
    case T:                                                                                                     \
        if constexpr (cfits(T, P, (int)sizeof(R), false, (int)(sizeof(Z) / sizeof(R)))) return launch<XS, Z, R, T, P>(a, nch, st); \
        break;
        MDSP_CREG_CASE(8)
        MDSP_CREG_CASE(16)
        MDSP_CREG_CASE(24)
        MDSP_CREG_CASE(32)
        MDSP_CREG_CASE(40)
        MDSP_CREG_CASE(48)
        MDSP_CREG_CASE(56)
        MDSP_CREG_CASE(64)
        MDSP_CREG_CASE(80)
        MDSP_CREG_CASE(96)
        MDSP_CREG_CASE(112)
#undef MDSP_CREG_CASE
        default: break;
    }
    MDSP_FAIL(MDSP_ERR_ASSERTION, "no complex register-tap instantiation for %d taps per phase, %d residues per thread", a.tp, P);
}
template <typename XS, typename Z, typename R> int dispatch_p(int P, FirRegArgs& a, int64_t nch, hipStream_t st) {
    return P == 2 ? dispatch_tpc<XS, Z, R, 2>(a, nch, st) : dispatch_tpc<XS, Z, R, 1>(a, nch, st);
}

}  // namespace

namespace mdsp {
bool fir_creg_ok(int x_dtype, bool acc_double, int64_t tp, int64_t L, int64_t M) { return cchoose_p(x_dtype, acc_double, tp, L, M) != 0; }
int fir_creg_run(int x_dtype, bool acc_double, FirRegArgs& a, int64_t nch, hipStream_t st) {
    const int P = cchoose_p(x_dtype, acc_double, a.tp, a.L, a.M);
    if (P == 0) MDSP_FAIL(MDSP_ERR_ASSERTION, "complex register-tap polyphase kernel: shape not instantiated");
    a.nrounds = cdiv(a.nout, (int64_t)a.L);
    switch (x_dtype) {
        case MDSP_F32: return acc_double ? dispatch_p<float, double, double>(P, a, nch, st) : dispatch_p<float, float, float>(P, a, nch, st);
        case MDSP_F64: return dispatch_p<double, double, double>(P, a, nch, st);
        case MDSP_C32: return acc_double ? dispatch_p<cx<float>, cx<double>, double>(P, a, nch, st) : dispatch_p<cx<float>, cx<float>, float>(P, a, nch, st);
        case MDSP_C64: return dispatch_p<cx<double>, cx<double>, double>(P, a, nch, st);
        default: MDSP_FAIL(MDSP_ERR_ASSERTION, "complex register-tap polyphase kernel: dtype %d", x_dtype);
    }
}
}  // namespace mdsp
