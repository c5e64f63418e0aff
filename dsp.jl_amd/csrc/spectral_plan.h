// The STFT plan object (opaque behind the C ABI; a multitaper plan embeds one) and the host functions that cross the spectral units: spectral.hip (routing,
// mdsp_frames, gx_run), welch.hip (mdsp_welch_*), stft.hip (mdsp_stft_*), spectral_gen.hip (the mixed-radix kernels of both), multitaper.hip (mdsp_mt_*)
// and hilbert.hip, which needs none of this.  The Welch plan object has its own header, welch_plan.h (comm.hip and hostpath.hip read it too).
// Internal to the library.
#pragma once

#include "common.h"
#include "chunk_units.h"
#include "rocfft_wrap.h"
#include "bigfft.h"
#include "gx_plan.h"
#include "spectral_ctcols.h"

struct mdsp_welch_plan_s;   // welch_plan.h

struct mdsp_stft_plan_s {
    int dtype = MDSP_F32, engine = MDSP_ENGINE_ROCFFT, onesided = 1, psd_only = 0;
    int route = MDSP_ROUTE_ROCFFT, r0 = 0;   // the kernel family exec runs, decided at creation (choose_spectral_route)
    int64_t n = 0, noverlap = 0, nfft = 0, nout = 0;
    double r = 1;
    bool have_win = false;
    mdsp::DevBuf win, table;
    const double* win_ptr = nullptr;   // window used by exec (the plan's own, or one taper of a multitaper plan)
    int accumulate = 0;                // PSD mode: out += |X|^2 m instead of out = (the taper loop of mt_pgram!, multitaper.jl:240-243)
    int mt_ntapers = 0;                // > 0: all tapers in one launch where the kernel supports it (real input, fused engine)
    const double* mt_rinv = nullptr;
    mdsp::RocPlan fwd;
    mdsp::DevBuf fr, spec;
    int64_t batch = 0;
    mdsp::big::EngineHolder big;       // nfft above the single-workgroup kernels: the multi-pass engine (bigfft.hip)
    mdsp::GxPlan gx;                   // 7-smooth sizes without a compile-time schedule: the run-time-schedule kernel (spectral_gx.h)
    mdsp::DevBuf winr;                 // lean compile-time schedules (CtSched flag 4096): the window of THIS launch in the working precision (multitaper plans change it per taper)
    mdsp::CtColsPlan ctbig;            // columns on the single-workgroup schedules of ctbig_sizes.h (spectral_ctbig_cols.hip)
};

namespace mdsp {
#pragma GCC visibility push(hidden)   // shared by the spectral units, not exported from the library
// spectral.hip
struct SpecRoute {
    int engine = MDSP_ENGINE_ROCFFT, route = MDSP_ROUTE_ROCFFT, r0 = 0;
};
int choose_spectral_route(int engine, int dtype, int64_t nfft, int kind, SpecRoute* out);   // kind 0: Welch sums, 1: columns
int check_split(int64_t n, int64_t noverlap, int64_t nfft);
bool lean_window_needed(int64_t nfft, bool dbl);
// stft.hip (multitaper.hip runs its tapers through the STFT plan it embeds)
int stft_dispatch(mdsp_stft_plan_s* plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_, void* out_dev, int64_t ldo, int64_t chs, hipStream_t st);
int prepare_stft_tables(mdsp_stft_plan_s* pl);
// spectral_gen.hip: the mixed-radix kernels, both modes.  gen_welch leaves *ngroups partial rows in pl->partial.
int gen_welch(mdsp_welch_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, int64_t K, int64_t hop, const double* win, hipStream_t st, int64_t* ngroups);
int gen_stft(mdsp_stft_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, void* out, int64_t ldo, int64_t chs, int64_t K, int64_t hop, const double* win,
             hipStream_t st);
// Intermediates (windowed frames + spectra) of one rocFFT-engine chunk: small enough to stay in the 256 MiB Infinity Cache
// between the three kernels that touch them, large enough that each launch fills the GPU.  MDSP_ROCFFT_CHUNK_MIB overrides.
inline int64_t rocfft_chunk_bytes() {
    return (int64_t)tunables().rocfft_chunk_mib << 20;   // default 192; swept 32..1024 MiB on config 4: 192 is 14 % faster than 64 (tools/rocfft_chunk_sweep.sh)
}
#pragma GCC visibility pop
}  // namespace mdsp
