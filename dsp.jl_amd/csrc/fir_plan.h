// The FIR filter objects (opaque behind the C ABI), the argument block every polyphase kernel family is launched from, and the few host functions that
// cross the FIR units: fir.hip (generic and Float32 register-tap kernels, dispatch, mdsp_fir_*), fir_mm.hip (matrix cores), fir_dec.hip (decimator),
// fir_arb.hip (FIRArbitrary) and tdfir.hip (time-domain FIR).  Internal to the library.
#pragma once

#include <cmath>

#include "common.h"

namespace mdsp {
struct FirArgs {
    const void* x;       // (xlen, nch), ld ldx, storage type XS
    const void* hist;    // (hl, nch) storage type XS
    void* y;             // (ycap, nch), ld ldy, type A
    const void* pfbT;    // tp * L taps (compute real type R, or cx<R> for complex taps), pfbT[i*L + phi]
    int64_t xlen, ldx, ldy, nout;
    int64_t phi0m1;      // phi0 - 1
    int64_t d0;          // input deficit (1-based first input index)
    int L, M, tp, hl;
    int tile;            // outputs per workgroup
    int span;            // LDS samples per tile (upper bound)
    int pfb_in_lds;
};
}  // namespace mdsp

struct mdsp_fir_s {
    int kind = 0;  // 0 standard, 1 interpolator, 2 decimator, 3 rational
    int64_t L = 1, M = 1, hlen = 0, tp = 0, hl = 0, nch = 1;
    int taps_dtype = MDSP_F32, x_dtype = MDSP_F32, out_dtype = MDSP_F32;
    bool acc_double = false;
    bool ctaps = false;   // complex taps: pfbT holds cx<R>, the output is complex for every signal type; generic or complex register-tap kernel (fir_creg.hip)
    int64_t phi_idx = 1, input_deficit = 1;  // the reference's 1-based state
    mdsp::DevBuf pfbT;
    mdsp::DevBuf hist[2];
    int cur = 0;
    bool exact = false;   // mdsp_fir_set_exact: the generic kernel only -- every output reads exactly its own tapsPerPhi-sample window (stream_filt.jl:496-509)
};

struct mdsp_firarb_s {
    mdsp_fir_s base;          // history buffers, dtypes, tp / hl / nch (kind = 4)
    double rate = 1.0, delta = 0.0;
    int64_t nphi = 32;
    // the reference's state (stream_filt.jl:96-104); phi_idx and alpha are functions of phi_acc
    double phi_acc = 0.0;
    int64_t input_deficit = 1, x_idx = 1;
    mdsp::DevBuf tab_x, tab_acc;
    mdsp::DevBuf prof;   // MDSP_ARB_PROF: per-workgroup clock stamps of the filtering kernel
    mdsp::DevBuf scan_t0, scan_wide, scan_E, scan_mind, scan_cb, scan_res;   // work space of the parallel trajectory scan (arb_scan.h)
    // trajectory cache: anchors of the last (phi_acc, input_deficit, xlen) evaluated
    bool cache_valid = false;
    double c_acc0 = 0.0;
    int64_t c_def0 = 0, c_xlen = -1, c_nout = 0, c_def_end = 0, c_xidx_end = 0;
    double c_acc_end = 0.0;
    int64_t n_scanned = 0, n_serial = 0;   // trajectories evaluated by the device scan / the serial host loop
};

namespace mdsp {
#pragma GCC visibility push(hidden)   // shared by the FIR units, not exported from the library
// fir.hip
bool fir_fast_ok(const mdsp_fir_s* f, int P);
int shiftin_dispatch(mdsp_fir_s* f, const void* x, int64_t xlen, int64_t ldx, hipStream_t st);
int fir_reset_on(mdsp_fir_s* f, hipStream_t st, bool async);
// Julia's round(Int, x): round half to even
inline int64_t round_half_even(double v) { return (int64_t)std::nearbyint(v); }
#pragma GCC visibility pop
}  // namespace mdsp
