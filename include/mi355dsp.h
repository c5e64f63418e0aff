/*
 * mi355dsp.h -- C ABI of libmi355dsp.so: DSP.jl's FFT-filtering / spectral-estimation hot path on MI355X.
 *
 * DSP.jl (v0.8.5) has no FFI of its own: the hot path leaves Julia only through AbstractFFTs plans
 * (FFTW) and BLAS.dot.  This header is the boundary a thin Julia `ccall` module (julia/MI355DSP.jl) or the
 * Python/ctypes host (dsp.jl_amd/) binds instead of those calls; every entry point below names the
 * reference routine whose inner loop it replaces (paths relative to DSP.jl `src/`).
 *
 * Conventions
 *   - Plain C: pointers, int64 sizes, int status.  Nothing throws or aborts.  0 = MDSP_OK, <0 = error class
 *     (the host wrapper maps classes to the same exception types DSP.jl raises); mdsp_last_error_string()
 *     returns a thread-local message.
 *   - `*_dev` pointers are device (HBM) pointers owned by the caller; `*_host` pointers are host memory read
 *     during the call.  Handles own plans, work buffers, tables and streaming state.  A handle is
 *     single-owner; calls are ordered on the `stream` argument (a hipStream_t passed as void*; NULL = the
 *     null stream).  Distinct handles may be used from distinct host threads.
 *   - Arrays are column-major: a multi-channel signal is (len, nch) with leading dimension `ld` (elements).
 *   - Lengths, offsets and phase indices are int64 and follow the reference's 1-based state values where the
 *     reference exposes them (phi_idx, input_deficit).
 */
#ifndef MI355DSP_H
#define MI355DSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDSP_VERSION 100 /* 0.1.0 */

/* status codes: error classes mirror the Julia exception types of the reference */
enum {
    MDSP_OK = 0,
    MDSP_ERR_ARGUMENT = -1,    /* ArgumentError      (dspbase.jl:28-33, filt.jl:474,531, periodograms.jl:396,564,876, stream_filt.jl:415,490) */
    MDSP_ERR_DOMAIN = -2,      /* DomainError        (periodograms.jl:44-45,397,565; stream_filt.jl:194,217) */
    MDSP_ERR_DIMENSION = -3,   /* DimensionMismatch  (periodograms.jl:255,735-737) */
    MDSP_ERR_ASSERTION = -4,   /* AssertionError     (stream_filt.jl:634,718,722) */
    MDSP_ERR_UNSUPPORTED = -5, /* valid in DSP.jl but outside this library's scope -> caller falls back to CPU */
    MDSP_ERR_DEVICE = -6,      /* HIP / rocFFT / RCCL runtime failure */
    MDSP_ERR_NOMEM = -7
};

/* element types (fftintype / fftouttype / fftabs2type rules, util.jl:92-104, are applied by the host) */
enum { MDSP_F32 = 0, MDSP_F64 = 1, MDSP_C32 = 2 /* ComplexF32 */, MDSP_C64 = 3 /* ComplexF64 */ };

/* transform engine */
enum {
    MDSP_ENGINE_AUTO = 0,  /* fused in-LDS FFT kernels when the size is supported, rocFFT otherwise */
    MDSP_ENGINE_FUSED = 1, /* segment/window -> FFT -> epilogue in ONE kernel, FFT held in LDS/registers */
    MDSP_ENGINE_ROCFFT = 2 /* segmenter / epilogue kernels around cached, batched rocFFT plans */
};

/* ------------------------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------------------------- */
int mdsp_version(void);
const char* mdsp_last_error_string(void);
/* Select the device for the calling thread and create the per-device context (rocFFT setup, plan cache). */
int mdsp_init(int device);
int mdsp_shutdown(void);
/* Fifteen optional environment variables (INTEGRATION.md "Environment": MDSP_ENGINE, MDSP_WG_PER_CU, MDSP_PLAN_CACHE_TOTAL / _IDLE, MDSP_ROCFFT_CHUNK_MIB,
 * MDSP_HOST_CHUNK_MIB, MDSP_BIG_CHUNK_MIB, MDSP_BIGFFT, MDSP_GX, MDSP_FIR_MM, MDSP_FIR_DEC, MDSP_FIR_EXACT, MDSP_ARB_SCAN, MDSP_ARB_SCAN_MIN,
 * MDSP_FIR_CHOICE_FILE) are read once, by mdsp_init() or on first use; exec and plan paths never call getenv.  mdsp_reload_tunables() re-reads them and is NOT
 * thread-safe against concurrent library calls (exec and plan paths read the table without a lock: tuning tools are single-threaded).
 * Everything that only steers an experiment -- kernel variants, tile shapes, wave priorities (about fifty names up to round 5) -- is a KNOB, not an environment
 * variable: mdsp_set_knob(name, value, 0) sets one, (name, 0, 1) puts its default back; used by tools/ and tests/ only.  mdsp_debug_knobs() is 1 only for a
 * library built with -DMDSP_DEBUG_KNOBS, which also reads every knob from the environment and carries the profiling switches (MDSP_ABLATE, ...). */
int mdsp_reload_tunables(void);
int mdsp_set_knob(const char* name, int value, int unset);
int mdsp_debug_knobs(void);
int mdsp_device_count(int* count);

/* Device-memory helpers for hosts without their own GPU array type (ctypes tests, the Julia wrapper). */
int mdsp_malloc(void** dev_ptr, size_t bytes);
int mdsp_free(void* dev_ptr);
int mdsp_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int mdsp_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int mdsp_memset(void* dst_dev, int value, size_t bytes, void* stream);
int mdsp_stream_synchronize(void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Pure index arithmetic (host; bit-exact with the reference)
 * ---------------------------------------------------------------------------------------------------- */
/* util.jl:134  nextfastfft(n) = nextprod((2,3,5,7), n) */
int64_t mdsp_nextfastfft(int64_t n);
/* dspbase.jl:268-291  optimalfftfiltlength(nb, nx) */
int64_t mdsp_optimal_fft_len(int64_t nb, int64_t nx);
/* periodograms.jl:49-50  number of frames of ArraySplit (trailing partial frame dropped) */
int64_t mdsp_frame_count(int64_t len, int64_t n, int64_t noverlap);
/* stream_filt.jl:317-322  outputlength(inputlength, L//M, initial_phi) */
int64_t mdsp_outputlength(int64_t inputlength, int64_t L, int64_t M, int64_t initial_phi);
/* stream_filt.jl:358-364  inputlength(outputlength, L//M, initial_phi, RoundDown|RoundUp) */
int64_t mdsp_inputlength(int64_t outputlength, int64_t L, int64_t M, int64_t initial_phi, int round_up);
/* Overlap-save block geometry of _fftfilt! (Filters/filt.jl:490,504-517) for block `iblock` (0-based):
 * off (1-based first output), npadbefore, xstart (1-based), n (samples copied), nout (samples saved). */
int mdsp_ols_block_geometry(int64_t nb, int64_t nx, int64_t nfft, int64_t iblock, int64_t* off,
                            int64_t* npadbefore, int64_t* xstart, int64_t* n, int64_t* nout);

/* ------------------------------------------------------------------------------------------------------
 * Overlap-save FIR filtering / convolution
 *   replaces the block loop of _fftfilt! (Filters/filt.jl:504-518: zero+copy, rfft, .* filterft, brfft, copy)
 *   and of unsafe_conv_kern_os! (dspbase.jl:546-606) incl. its padded edge blocks (:371-486), N = 1.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_ols_plan_s* mdsp_ols_plan;
enum {
    MDSP_OLS_FILT = 0, /* y has the length of x; taps pre-scaled by 1/nfft            (filt.jl:499) */
    MDSP_OLS_CONV = 1  /* y has length nx+nb-1; filter SPECTRUM scaled by 1/nfft (dspbase.jl:516) */
};
/* taps_host: nb elements of `dtype` (real taps for MDSP_F32/F64, complex for MDSP_C32/C64).
 * nfft = 0 selects mdsp_optimal_fft_len(nb, nx_hint). */
int mdsp_ols_plan_create(mdsp_ols_plan* plan, const void* taps_host, int64_t nb, int64_t nfft, int64_t nx_hint,
                         int dtype, int mode, int engine);
int mdsp_ols_plan_destroy(mdsp_ols_plan plan);
int mdsp_ols_plan_info(mdsp_ols_plan plan, int64_t* nfft, int64_t* block_len /* L */, int* engine_used);
/* What actually executes.  mdsp_ols_plan_info reports the REFERENCE's geometry (the nfft optimalfftfiltlength / the caller chose, dspbase.jl:268-291);
 * the fused engine runs it as it is up to nfft = 8192 (4096 in Float64).  Longer filters -- ~1100 taps and more, where the reference asks for
 * nfft = 16384 ... 2^20 -- are re-blocked: one block of the largest in-LDS transform while the filter covers at most half of it, else a
 * uniformly partitioned filter (2..4 partitions of exec_nfft/2 taps, spectra of the last blocks kept in registers).  Beyond four partitions
 * (more than 16384 Float32 / 8192 Float64 taps, any of the four dtypes) a block no longer fits a workgroup and is transformed in passes over HBM
 * (partitions = 1): exec_nfft = R0 x S with S the longest single-workgroup transform (8192 / 4096) -- a column pass of R0-point
 * transforms, ONE kernel per row for transform, filter spectrum, inverse transform and twiddle, a column pass back (R0 = 64 up to S x 16 taps, 256 up
 * to S x 64) -- and beyond that three passes each way on natural-order spectra (2^20 points and more).  Same outputs within rounding, one plan for
 * every filter length with 2 nb <= 2^26. */
int mdsp_ols_plan_geometry(mdsp_ols_plan plan, int64_t* exec_nfft, int64_t* exec_block_len, int* partitions);
/* The same answer without a plan and without a device (pure host arithmetic: what mdsp_ols_plan_create WOULD execute for these arguments, so a host
 * can size a time-axis split or a test can check the rule on a machine without a GPU).  engine_used: MDSP_ENGINE_*; rows: > 0 when the blocks run in
 * the rows form of the multi-pass engine (R0 rows of 8192 / 4096 points), else 0.  Any output pointer may be NULL. */
int mdsp_ols_geometry_for(int64_t nb, int64_t nfft, int64_t nx_hint, int dtype, int mode, int engine, int64_t* exec_nfft, int64_t* exec_block_len,
                          int* partitions, int* engine_used, int* rows);
/* The windows mdsp_ols_exec and mdsp_ols_exec_host run: tile_len outputs each, starting tile_lead samples in front of their first output.
 * Everywhere tile_len == exec_block_len and tile_lead == nb - 1, except on TILED plans -- real Float32, fused engine, exec_nfft 2048, 249 .. 257 taps:
 * (1792, 256), so that every window starts a multiple of 1 KiB into the column and the overlap of neighbouring windows stays in registers.  The
 * filter spectrum and the geometry the calls above report do not change; outputs agree with the untiled windows within rounding.  The knob
 * MDSP_OLS_TILE = 0 (mdsp_set_knob, before the plan is made) switches the rule off.  mdsp_ols_tile_for: the same answer without a plan or a device. */
int mdsp_ols_plan_tile(mdsp_ols_plan plan, int64_t* tile_len, int64_t* tile_lead);
int mdsp_ols_tile_for(int64_t nb, int64_t nfft, int64_t nx_hint, int dtype, int mode, int engine, int64_t* tile_len, int64_t* tile_lead);
/* The cache policy of a tiled plan's launches: *streaming = 1 when a whole-column call over `columns` columns of nx samples / nout outputs
 * runs the kernel whose loads and stores bypass the caches (same arithmetic, bit-identical outputs).  Knob MDSP_OLS_STREAM (mdsp_set_knob, read at launch):
 * 1 = the footprint rule (the default) -- launches that read and write more than 512 MiB, (nx + nout) columns 4 bytes, which nothing can still hold in
 * cache for a consumer --, 0 = never, 2 = every launch of a tiled plan.  Always 0 for dtypes that have no tiled plans and under MDSP_OLS_TILE = 0.  No device. */
int mdsp_ols_stream_for(int64_t nx, int64_t nout, int64_t columns, int dtype, int* streaming);
/* The run schedule of the fused kernel's persistent grid: a launch of `units` units (pairs of real blocks, complex blocks) on `slots`
 * transform slots gives every slot runs of *run_len consecutive units, run r of slot s at unit (r slots + s) run_len, and *niter iterations in all (the
 * same for every slot).  streaming_tiled != 0: the streaming launch of a tiled plan, which walks runs of 2 units from 65536 units on; every other launch walks
 * one run per slot, *run_len = ceil(units / slots).  Outputs are bit-identical under every schedule.  Knobs (mdsp_set_knob, read at launch): MDSP_OLS_RUN_LEN = n > 0 forces
 * runs of n units (never longer than one run per slot), MDSP_RUNS_PER_SLOT != 1 that many runs per slot.  No device. */
int mdsp_ols_run_for(int64_t units, int64_t slots, int streaming_tiled, int64_t* run_len, int64_t* niter);
/* x_dev: (nx, ncols) ld ldx;  y_dev: (nout, ncols) ld ldy.  nout = nx (filt), nx+nb-1 (conv), or any
 * 0 <= nout <= nx+nb-1.  x and y must not alias (Filters/filt.jl:438-439). */
int mdsp_ols_exec(mdsp_ols_plan plan, const void* x_dev, int64_t nx, int64_t ncols, int64_t ldx, void* y_dev,
                  int64_t nout, int64_t ldy, void* stream);
/* Blocks [first_block, first_block + nblocks_range) of the SAME block grid mdsp_ols_exec uses for one column of nx samples /
 * nout outputs, from a slice of the signal: xs_dev holds x[xs_first .. xs_first + xs_len) and must cover the samples those blocks
 * read, [first_block L - (nb-1), (first_block + nblocks_range) L) clipped to [0, nx); ys_dev[0..] receives the outputs from
 * first_block L on (L = exec_block_len of mdsp_ols_plan_geometry).  first_block must be even for real dtypes on single-block plans
 * (bit-identical to the whole-column call when mdsp_ols_plan_tile reports tile_len == exec_block_len, within rounding on tiled plans, whose
 * block ranges run the untiled windows and never read in front of the slice); partitioned plans (long filters) take any first_block and agree
 * with the whole-column call within rounding.  Building block of mdsp_ols_exec_host and of a time-axis split
 * of one stream over GPUs (no collective: overlap-save blocks are independent, Filters/filt.jl:504-518). */
int mdsp_ols_exec_range(mdsp_ols_plan plan, const void* xs_dev, int64_t xs_first, int64_t xs_len, int64_t nx, void* ys_dev,
                        int64_t first_block, int64_t nblocks_range, int64_t nout, void* stream);
/* Segmenter only (K1): materialise blocks [first_block, first_block+nblocks) of column 0 as (nfft, nblocks)
 * -- the exact contents of `tmp1` before the forward transform (filt.jl:509-510).  For parity tests. */
int mdsp_ols_segment(mdsp_ols_plan plan, const void* x_dev, int64_t nx, int64_t first_block, int64_t nblocks,
                     void* seg_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Framing (ArraySplit), Welch, STFT / spectrogram / periodogram
 *   replaces ArraySplit getindex (periodograms.jl:57-69), mul!(outbuf, plan, sig) (:754,:888),
 *   fft2pow! (:142-172) and fft2oneortwosided! (:234-244).
 * ---------------------------------------------------------------------------------------------------- */
/* K4 only: frames [first, first+count) of one channel as (nfft, count) of the signal's fftintype, windowed
 * in Float64 and rounded once, zero tail -- bit-identical to the reference's buffer contents. */
int mdsp_frames(const void* s_dev, int64_t len, int dtype, int64_t n, int64_t noverlap, int64_t nfft,
                const double* window_host /* n doubles or NULL */, int64_t first, int64_t count, void* frames_dev,
                void* stream);

typedef struct mdsp_welch_plan_s* mdsp_welch_plan;
/* dtype: element type of the signal (fftintype already applied).  window_host: n Float64 or NULL.
 * r = fs * sum(abs2, window) (or fs * n without window), as WelchConfig computes it (periodograms.jl:567-568).
 * onesided requires a real dtype (ArgumentError otherwise, :564). */
int mdsp_welch_plan_create(mdsp_welch_plan* plan, int64_t n, int64_t noverlap, int64_t nfft,
                           const double* window_host, double r, int onesided, int dtype, int engine);
int mdsp_welch_plan_destroy(mdsp_welch_plan plan);
int mdsp_welch_plan_info(mdsp_welch_plan plan, int64_t* nout, int* engine_used);
/* s_dev: (len, nch) ld lds.  psd_dev: (nout, nch) ld ldp of fftabs2type(dtype); nout = nfft/2+1 or nfft.
 * Each channel gets its own PSD (welch_pgram_helper!, periodograms.jl:746-759). */
int mdsp_welch_exec(mdsp_welch_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds,
                    void* psd_dev, int64_t ldp, void* stream);
/* Streaming form of the same computation -- mdsp_welch_exec IS reset + accumulate + finalize.  The plan owns Float64 sums of
 * |X[k]|^2 over every frame accumulated since the last reset; a long stream may be handed over slice by slice (each slice: whole
 * frames, i.e. consecutive slices overlap by n - hop samples), by several ranks (mdsp_welch_allreduce), or from host memory
 * (mdsp_welch_exec_host).  finalize forms psd = fold(sums) / (K fs sum(w^2)) with K = frames_total (0: the frames accumulated here),
 * periodograms.jl:751-757.  All slices of one accumulation must have the same channel count. */
int mdsp_welch_reset(mdsp_welch_plan plan);
int mdsp_welch_accumulate(mdsp_welch_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds, void* stream);
int mdsp_welch_frames_accumulated(mdsp_welch_plan plan, int64_t* frames_per_channel);
int mdsp_welch_finalize(mdsp_welch_plan plan, int64_t frames_total, void* psd_dev, int64_t ldp, void* stream);
/* The accumulator itself (Float64, `count` values, layout private to the engine): what a caller-side collective would sum over ranks. */
int mdsp_welch_accumulator(mdsp_welch_plan plan, void** acc_dev, int64_t* count);
/* Local part of the cross-channel mean: sum over nch rows (ld ldp) of nout values, in `real_dtype`, into sum_dev (nout). */
int mdsp_channel_sum(const void* psd_dev, int64_t nout, int64_t nch, int64_t ldp, int real_dtype, void* sum_dev,
                     void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, channels sharded over ranks, RCCL over xGMI for the ONE collective of the path.
 *   The reference loops over columns / channels serially (Filters/filt.jl:504, stream_filt.jl:768 `mapslices`); here rank r owns
 *   a contiguous block of channels and runs the single-GPU entry points on them -- no data-path collective -- and only the
 *   cross-channel Welch mean needs an exchange: an all-reduce (sum) of nout values.
 *   Bootstrap: rank 0 calls mdsp_comm_unique_id and ships the 128 bytes to the other ranks by whatever the host has (MPI.jl bcast,
 *   a shared file, torch.distributed's store); every rank then calls mdsp_comm_init_rank (collective) after mdsp_init(device).
 *   librccl is bound at run time; without it these entries return MDSP_ERR_DEVICE and everything else keeps working.
 * ---------------------------------------------------------------------------------------------------- */
#define MDSP_COMM_ID_BYTES 128
typedef struct mdsp_comm_s* mdsp_comm;
int mdsp_comm_unique_id(void* id128 /* MDSP_COMM_ID_BYTES, host */);
int mdsp_comm_init_rank(mdsp_comm* comm, const void* id128, int rank, int nranks);
int mdsp_comm_destroy(mdsp_comm comm);
int mdsp_comm_info(mdsp_comm comm, int* rank, int* nranks);
/* in-place sum over ranks of `count` Float32 / Float64 values (ncclAllReduce on `stream`) */
int mdsp_allreduce_sum(mdsp_comm comm, void* buf_dev, int64_t count, int real_dtype, void* stream);
/* Cross-channel Welch mean: psd_dev = this rank's per-channel PSDs (nch_local rows of ld ldp, plan's nout bins, fftabs2type);
 * mean_dev (nout) = (1 / nch_total) * sum over the channels of ALL ranks.  comm == NULL or a 1-rank communicator: local mean. */
int mdsp_welch_mean_allreduce(mdsp_welch_plan plan, const void* psd_dev, int64_t nch_local, int64_t ldp, int64_t nch_total,
                              void* mean_dev, mdsp_comm comm, void* stream);
/* ONE stream split along time over ranks: sums the plans' Float64 accumulators and frame counts over ranks in place; a following
 * mdsp_welch_finalize(plan, 0, ...) gives every rank the PSD of the whole stream.  Stream-ordered (one RCCL group of the sums and the
 * frame count; the total count stays on the device and finalize reads it there); mdsp_welch_frames_accumulated afterwards reads it back. */
int mdsp_welch_allreduce(mdsp_welch_plan plan, mdsp_comm comm, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Host-array entry points: DSP.jl's own call shape (host Arrays in, host Arrays out; Filters/filt.jl:458-476,
 * periodograms.jl:647-744, :872-897, stream_filt.jl:627-637, :688-775) as a chunked H2D || kernel || D2H pipeline: one internal stream per
 * PCIe direction plus one for the kernels, three lanes of device (and, for pageable arrays, page-locked staging) buffers, so that chunk k's
 * download, chunk k+1's kernels and chunk k+2's upload are in flight together (full duplex).
 * Synchronous (results are in the host arrays on return); PCIe-bound -- see DESIGN.md section 5 for the measured rates.
 *   flags: MDSP_HOST_PINNED = the caller's arrays are already page-locked (mdsp_host_alloc / mdsp_host_register): no staging copies.
 *   Chunk size: MDSP_HOST_CHUNK_MIB (default 64).  Overlap-save results are bit-identical to the device-resident calls for single-block
 *   plans (same block grid); PARTITIONED (long-filter) plans run block ranges from slices of the signal (mdsp_ols_exec_range: samples under
 *   the zero taps in front of a slice read as zero), so they equal the whole-column call within rounding, and a NaN / Inf earlier in the
 *   stream does not propagate into later slices the way it does through the device-resident delay line.  Welch: equal up to Float64
 *   summation order.
 *   Ordering and resources: every host-array call starts with a device-wide synchronisation (the pipeline's streams are non-blocking; this
 *   orders them behind whatever the same handle has queued on other streams); one pipeline per device, guarded by a mutex for the whole
 *   call -- host-array calls of several threads on one device run one after the other; its three lanes of device (and page-locked staging)
 *   buffers only grow and stay until mdsp_host_pipeline_trim() or mdsp_shutdown().  mdsp_fir_exec_host advances the filter state chunk by
 *   chunk: after an error return the filter's state is unspecified -- mdsp_fir_reset (or set_state) before using it again.
 * ---------------------------------------------------------------------------------------------------- */
#define MDSP_HOST_PINNED 1
/* frees the host pipelines' device and page-locked buffers of every device (they are re-grown on the next host-array call) */
int mdsp_host_pipeline_trim(void);
int mdsp_host_alloc(void** host_ptr, size_t bytes);      /* hipHostMalloc */
int mdsp_host_free(void* host_ptr);
int mdsp_host_register(void* host_ptr, size_t bytes);    /* hipHostRegister: page-lock an existing allocation (e.g. a Julia Array) */
int mdsp_host_unregister(void* host_ptr);
int mdsp_ols_exec_host(mdsp_ols_plan plan, const void* x_host, int64_t nx, int64_t ncols, int64_t ldx, void* y_host, int64_t nout,
                       int64_t ldy, int flags);
int mdsp_welch_exec_host(mdsp_welch_plan plan, const void* s_host, int64_t len, int64_t nch, int64_t lds, void* psd_host,
                         int64_t ldp, int flags);
/* stft / spectrogram / periodogram of host arrays (mdsp_stft_exec with host pointers, periodograms.jl:872-897): channel by channel in runs of
 * whole frames, the chunk sized by its OUTPUT (2-8x the input); bit-identical to the device-resident call.  Declared after mdsp_stft_plan below. */

typedef struct mdsp_stft_plan_s* mdsp_stft_plan;
/* psd_only = 0: raw STFT columns (fftouttype), unnormalised (periodograms.jl:892);
 * psd_only = 1: spectrogram columns fft2pow!(…, r, onesided, offset) (:890) in fftabs2type.
 * periodogram(s) (periodograms.jl:393-417) is the single-frame case n = length(s), noverlap = 0, psd_only = 1. */
int mdsp_stft_plan_create(mdsp_stft_plan* plan, int64_t n, int64_t noverlap, int64_t nfft,
                          const double* window_host, double r, int onesided, int psd_only, int dtype, int engine);
int mdsp_stft_plan_destroy(mdsp_stft_plan plan);
int mdsp_stft_plan_info(mdsp_stft_plan plan, int64_t* nout, int* engine_used);
/* s_dev: (len, nch) ld lds.  out_dev: nch matrices (nout, k) column-major with column stride ldo (>= nout)
 * and channel stride chs (elements of the output type). */
int mdsp_stft_exec(mdsp_stft_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds, void* out_dev,
                   int64_t ldo, int64_t chs, void* stream);
/* the same with host arrays (see "Host-array entry points" above); flags: MDSP_HOST_PINNED */
int mdsp_stft_exec_host(mdsp_stft_plan plan, const void* s_host, int64_t len, int64_t nch, int64_t lds, void* out_host,
                        int64_t ldo, int64_t chs, int flags);

/* Kernel family a Welch / STFT / multitaper plan runs (decided once, at plan creation, from the tunables of that moment) */
enum {
    MDSP_ROUTE_ROCFFT = 0,     /* the rocFFT pipeline (engine_used = MDSP_ENGINE_ROCFFT) */
    MDSP_ROUTE_POW2 = 1,       /* register-resident power-of-two kernels (256 .. 8192 Float32, .. 4096 Float64) */
    MDSP_ROUTE_GEN = 2,        /* mixed-radix LDS kernel and its compile-time schedules */
    MDSP_ROUTE_GX = 3,         /* run-time-schedule single-workgroup kernel */
    MDSP_ROUTE_CTBIG = 4,      /* Welch sums on a single-workgroup compile-time schedule */
    MDSP_ROUTE_CTBIG_COLS = 5, /* STFT columns on a single-workgroup compile-time schedule */
    MDSP_ROUTE_CTCOLS_BIG = 6, /* Welch sums, nfft = r0 x a compile-time row of 8193 .. 16384 points */
    MDSP_ROUTE_CTCOLS_F64 = 7, /* Welch sums, nfft = r0 x a Float64 compile-time row of 4097 .. 9600 points */
    MDSP_ROUTE_CTCOLS = 8,     /* Welch sums, nfft = r0 x a compile-time row (mixed-radix schedules) */
    MDSP_ROUTE_CTROWS = 9,     /* Welch sums, nfft = r0 x S in two kernels (column kernel, then single-workgroup rows) */
    MDSP_ROUTE_BIG = 10        /* multi-pass engine */
};
/* Pure host arithmetic, no device needed (like mdsp_ols_geometry_for): what mdsp_welch_plan_create (kind = 0) or mdsp_stft_plan_create /
 * mdsp_mt_plan_create (kind = 1) WOULD record for these arguments under the current tunables -- the engine, the route (MDSP_ROUTE_*) and the
 * column factor r0 of the CTCOLS* / CTROWS routes (0 otherwise).  Fails with the status and message plan creation would.  Any output pointer may be NULL. */
int mdsp_spectral_route_for(int kind, int dtype, int64_t nfft, int engine, int* engine_used, int* route, int* r0);

/* The engine loops that cut their work into chunks so that the intermediates stay within a memory budget */
enum {
    MDSP_CHUNK_ROCFFT_WELCH = 0, /* rocFFT Welch: a unit is a frame of a channel, n = nfft; budget MDSP_ROCFFT_CHUNK_MIB (default 192) */
    MDSP_CHUNK_ROCFFT_STFT = 1,  /* rocFFT STFT / spectrogram / periodogram / multitaper: the same */
    MDSP_CHUNK_ROCFFT_OLS = 2,   /* rocFFT overlap-save: a unit is a block of a column, n = nfft; 64 MiB */
    MDSP_CHUNK_HILBERT = 3,      /* hilbert: a unit is a column of n points (real dtypes); 256 MiB */
    MDSP_CHUNK_BIG_SPECTRAL = 4, /* multi-pass engine, Welch sums (three passes or the rows form) and columns: a unit is a transform of n = nfft points -- two real
                                    frames, one complex frame; budget MDSP_BIG_CHUNK_MIB (default 1024) */
    MDSP_CHUNK_BIG_OLS = 5,      /* multi-pass overlap-save on natural-order spectra: a unit is a transform of n = exec_nfft points (two real blocks, one complex
                                    block) and takes two buffers of the same budget */
    MDSP_CHUNK_BIG_OLS_ROWS = 6  /* multi-pass overlap-save in the rows form: one buffer */
};
/* Pure host arithmetic, no device needed (like mdsp_ols_geometry_for): how many of `units` units the loop `kind` (MDSP_CHUNK_*) takes per chunk under the
 * current tunables -- the value the loop itself computes, at least 1 and at most max(units, 1); the loop then runs ceil(units / *units_per_chunk) chunks, the
 * last one with what is left.  dtype: the signal's.  units_per_chunk may be NULL. */
int mdsp_chunk_units_for(int kind, int dtype, int64_t n, int64_t units, int64_t* units_per_chunk);

/* ------------------------------------------------------------------------------------------------------
 * 2-D periodogram (periodograms.jl:473-509, kernels fft2pow2! / fft2pow2radial! :175-232)
 *   periodogram(s::AbstractMatrix{<:Real}; nfft = (nfft1, nfft2), fs, radialsum, radialavg) of a real (n1, n2) matrix:
 *   ptype 0  out (nfft1, nfft2) = abs2.(fft(s zero-padded to nfft)) / (fs n1 n2)     (norm2 = length(s), :488)
 *   ptype 1  radialsum: out (kmax) with kmax = min(nfft1, nfft2) / 2 + 1, the wave-number bins of :191-225
 *   ptype 2  radialavg: the same divided by the wave counts wc
 *   Output element type fftabs2type: Float32 for Float32 input, else Float64.  dtype: MDSP_F32 / MDSP_F64 (fftintype applied by the
 *   caller).  engine goes to the plan's two internal STFT plans (rows, then columns); engine_used reports the engine both took, or
 *   MDSP_ENGINE_AUTO when they took different ones.  Checks, before any device work, in the reference's order: nfft >= size(s)
 *   (MDSP_ERR_ARGUMENT "nfft must be >= size(s)"), n1 > 1 && n2 > 1, ptype in 0..2, dtype real.  fs must be positive (the internal
 *   column plan's normalisation).  The radial reduction uses no atomics: one plan gives bit-identical results exec after exec.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_periodogram2_plan_s* mdsp_periodogram2_plan;
int mdsp_periodogram2_plan_create(mdsp_periodogram2_plan* plan, int64_t n1, int64_t n2, int64_t nfft1, int64_t nfft2,
                                  double fs, int ptype, int dtype, int engine);
int mdsp_periodogram2_plan_destroy(mdsp_periodogram2_plan plan);
int mdsp_periodogram2_plan_info(mdsp_periodogram2_plan plan, int64_t* nout /* nfft1*nfft2 or kmax */,
                                int64_t* workspace_bytes, int* engine_used);
/* s_dev: (n1, n2), column stride lds >= n1.  out_dev: (nfft1, nfft2), column stride ldo >= nfft1 (ptype 0; rows nfft1 .. ldo-1 are not
 * written), or kmax values (ptype 1 / 2; ldo unused). */
int mdsp_periodogram2_exec(mdsp_periodogram2_plan plan, const void* s_dev, int64_t lds, void* out_dev, int64_t ldo, void* stream);
/* Pure host arithmetic, no device needed (like mdsp_ols_geometry_for): kmax, the wave counts wc (kmax values, may be NULL) and the
 * number of Float64 row partials of the radial reduction (the sum over rows of each row's bin range).  nfft1, nfft2 >= 2. */
int mdsp_periodogram2_geometry_for(int64_t nfft1, int64_t nfft2, int64_t* kmax, int64_t* wc_host, int64_t* partials);

/* ------------------------------------------------------------------------------------------------------
 * unwrap / unwrap! along one dimension (src/unwrap.jl:17-34, `dims::Integer`): accumulate!(unwrap_kernel(range), y, m; dims)
 *   y[0] = m[0],  y[i] = m[i] - round((m[i] - y[i-1]) / range) * range   along j of an (inner, len, outer) array, element (i, j, o) at
 *   i + inner (j + len o): a Julia array unwrapped along dimension d has inner = prod(size[1:d-1]), len = size[d], outer = prod(size[d+1:end]);
 *   a C-ordered array the same with the axes read from the last to the first.  No transposes: inner == 1 is the contiguous route
 *   (MDSP_UNWRAP_CONTIGUOUS), inner > 1 the strided one (MDSP_UNWRAP_STRIDED, coalesced across inner).
 *   Evaluated as an integer prefix sum K of d_i = rint((m[i] - m[i-1]) / range), y[i] = m[i] - T(K_i) range, every operation rounded in T as
 *   the reference's: bit-identical to the serial recurrence whenever no (m[i] - m[i-1]) / range lies near a rounding tie; near a tie the two
 *   forms may differ by whole periods from that sample on.  Documented range |K| < 2^24 (Float32) / 2^53 (Float64);
 *   beyond it the result is unspecified (the reference's own K no longer holds integers), the call stays inside its arrays.  A non-finite
 *   m[i], i >= 1, makes the rest of its line NaN, m[0] = NaN the whole line, m[0] = +-Inf followed by finite samples a line of +-Inf.
 *   dtype MDSP_F32 / MDSP_F64; range is converted to that type and must be finite and nonzero there.  segments: 0 = the library cuts a line
 *   into S segments when the lines alone do not fill the device; > 0 forces the cut (clamped to len; 1 when len <= 2; segments are
 *   ceil(len / segments) long, the last one ragged, and S counts the non-empty ones).  S == 1 is one launch; S > 1 three launches on the
 *   caller's stream (segment sums, carries, apply) and 24 bytes of workspace per segment and line.  No atomics and no waiting between
 *   workgroups: one plan gives bit-identical results exec after exec, and every cut gives the same bits.
 *   Checks, before any launch: sizes < 0, a dtype that is not real floating, range non-finite or 0: MDSP_ERR_ARGUMENT; any size == 0 succeeds
 *   without a launch; len == 1 is a copy.
 * ---------------------------------------------------------------------------------------------------- */
enum { MDSP_UNWRAP_CONTIGUOUS = 0, MDSP_UNWRAP_STRIDED = 1 };
typedef struct mdsp_unwrap_plan_s* mdsp_unwrap_plan;
int mdsp_unwrap_plan_create(mdsp_unwrap_plan* plan, int64_t inner, int64_t len, int64_t outer, int dtype, double range, int64_t segments);
int mdsp_unwrap_plan_destroy(mdsp_unwrap_plan plan);
int mdsp_unwrap_plan_info(mdsp_unwrap_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* workspace_bytes);
/* out_dev == in_dev is unwrap!(m); any other overlap of the two arrays is MDSP_ERR_ARGUMENT. */
int mdsp_unwrap_exec(mdsp_unwrap_plan plan, const void* in_dev, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed: the route, S, the segment length and the workspace a plan for these arguments has.  Any output
 * pointer may be NULL. */
int mdsp_unwrap_geometry_for(int64_t inner, int64_t len, int64_t outer, int dtype, int64_t segments, int* route, int64_t* nsegments,
                             int64_t* seglen, int64_t* workspace_bytes);
/* Host emulation of the device code (no device): the same geometry and the same operator and per-segment walk (csrc/unwrap_scan.h) on host
 * arrays, the three steps one after the other.  out_host may be in_host. */
int mdsp_unwrap_emulate_host(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int dtype, double range,
                             int64_t segments);

/* ------------------------------------------------------------------------------------------------------
 * filt / filt! for Biquad and SecondOrderSections (Filters/filt.jl:35-92), the stateful DF2TFilter forms (:188-210) and the two passes of
 * filtfilt (:341-360): a cascade of K second-order sections along the first dimension of n x ncols columns, ld elements apart.
 *   coef: K x 5 doubles, b0 b1 b2 a1 a2 per section (a0 = 1), rounded to the working type's real type before anything else.  has_gain != 0:
 *   the output of the last section is multiplied by gain (SecondOrderSections); has_gain == 0: it is the output (Biquad).
 *   dtype is the WORKING type promote_type(T, G, S) of the reference: MDSP_F32 / F64, or MDSP_C32 / C64 for a complex signal, whose columns
 *   are filtered as two real lines of element stride 2 (the coefficients are real).  x, y and state are arrays of that type.
 *   Per sample and section: y = fma(b0, x, s1); s1 = fma(a1, -y, fma(b1, x, s2)); s2 = fma(b2, x, -a2 * y), every operation rounded once in the
 *   working type.  Given the state at its first sample, every run of 16 samples is computed by exactly this serial recurrence; a scan with
 *   powers of the cascade's 2K x 2K state matrix (host, long double, rounded once) supplies the start states (csrc/sos_scan.h).
 *   state_dev: (2, K, ncols) values of the working type, element s + 2 (k + K c): read as the state in front of the first sample, overwritten with
 *   the state behind the last; NULL: zero state, end state dropped.  reverse != 0 walks every column from its last sample to its first (reads
 *   x[n-1-i], writes y[n-1-i]).  y_dev == x_dev with ldy == ldx filters in place; any other overlap is MDSP_ERR_ARGUMENT.
 *   segments as for unwrap: 0 = automatic, > 0 forced (clamped to n); S == 1 is one launch, S > 1 three (end states, carries, apply) with
 *   2 K values of workspace per segment and line.  tile = 64 run samples.  No atomics, nothing waits: results depend on the arguments only
 *   and equal mdsp_sos_emulate_host bit for bit.
 *   Checks, before any launch: negative sizes, nsections < 1, a bad dtype, non-finite coefficients or gain, ld < n, a partial overlap:
 *   MDSP_ERR_ARGUMENT.  nsections > 16, a section with a pole of modulus above 1 (its carry matrices grow without bound; poles ON the unit
 *   circle run), or carry matrices that overflow the working type: MDSP_ERR_UNSUPPORTED.  n == 0 or ncols == 0 succeeds without a launch.
 *   A plan touches the device at its first exec, not at creation: that call allocates and copies the carry matrices with a blocking hipMemcpy, so
 *   a plan's FIRST exec must not be inside a stream capture (later ones only launch kernels).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_sos_plan_s* mdsp_sos_plan;
int mdsp_sos_plan_create(mdsp_sos_plan* plan, const double* coef, int64_t nsections, double gain, int has_gain, int dtype, int64_t n, int64_t ncols,
                         int64_t segments);
int mdsp_sos_plan_destroy(mdsp_sos_plan plan);
int mdsp_sos_plan_info(mdsp_sos_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run, int64_t* workspace_bytes);
int mdsp_sos_exec(mdsp_sos_plan plan, const void* x_dev, int64_t ldx, void* y_dev, int64_t ldy, void* state_dev, int reverse, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_sos_geometry_for(int64_t nsections, int dtype, int64_t n, int64_t ncols, int64_t segments, int64_t* nsegments, int64_t* seglen,
                          int64_t* tile, int64_t* run, int64_t* workspace_bytes);
/* Host emulation of the device code (no device): the same cut, tiles, scan order and arithmetic (csrc/sos_scan.h) on host arrays. */
int mdsp_sos_emulate_host(const void* x_host, int64_t ldx, void* y_host, int64_t ldy, void* state_host, const double* coef, int64_t nsections,
                          double gain, int has_gain, int dtype, int64_t n, int64_t ncols, int64_t segments, int reverse);

/* ------------------------------------------------------------------------------------------------------
 * freqresp / phaseresp / grpdelay (Filters/response.jl:27-52, :73-76, :96-111) of a :z-domain filter with real coefficients: a rational function
 * evaluated at nw points of the unit circle, a lane per point (csrc/resp_op.h).
 *   dtype: MDSP_F32 or MDSP_F64, the REAL type of the working type (ComplexF32 / ComplexF64).  Every coefficient is rounded to it first.
 *   form MDSP_RESP_POLY:      num(y) / den(y), num = sum num[k] y^k (nnum >= 1), den = sum den[k] y^k, or 1 when nden == 0; Horner from the highest
 *                             coefficient.  MDSP_RESP_DERIV: coefficient k of the numerator is k * num[k], the product rounded once (response.jl:106);
 *                             den == num with nden == nnum is one device array (what grpdelay passes).  gain is not used.
 *        MDSP_RESP_SECTIONS:  gain * prod_k biquad_k(x), left to right from one; num: nnum x 5 doubles b0 b1 b2 a1 a2 (0 <= nnum <= 16), nden == 0;
 *                             biquad(x) = fma(fma(b0, x, b1), x, b2) / fma(x + a1, x, a2) (response.jl:49-52).
 *        MDSP_RESP_ZPK:       (gain * prod (x - z_i)) / prod (x - p_i) (response.jl:47-48); num: nnum zeros, den: nden poles, (re, im) pairs of doubles.
 *   out_mode MDSP_RESP_COMPLEX: H, nw complex values; MDSP_RESP_ANGLE: atan2(im H, re H), nw real values; MDSP_RESP_REAL_MINUS: re H - cminus, nw real
 *   values.  in_mode MDSP_RESP_W: nw real w, the point is e^{iw}, with MDSP_RESP_NEG e^{-iw} (the device's sincos); MDSP_RESP_POINTS: nw complex points
 *   as given (any contour; the mode in which the device equals mdsp_resp_emulate_host bit for bit for the COMPLEX and REAL_MINUS outputs).
 *   The division is Smith's scaled one with correctly rounded real divisions; every other operation is an fma, a product, a sum or a difference
 *   rounded once.
 *   The cut (POLY only): the coefficients go in C chunks of L = 2^l; one launch over (tiles of 64 points x chunks) stores every chunk's Horner value
 *   into the plan's workspace, a second forms q = y^L by l squarings per point (in double-word arithmetic, rounded once), runs Horner over the chunks in q from the highest, divides and
 *   stores.  Store first, sum afterwards: no atomics, nothing waits, results depend on the arguments only.  chunks: 0 = automatic (C = 1 unless the
 *   points alone leave the device empty), > 0 forced: L = the power of two >= ceil(n / chunks), at least 16, C = ceil(n / L); C == 1 is a single
 *   launch without a workspace.  SECTIONS and ZPK are never cut (chunks is checked and otherwise ignored).
 *   Checks, before any launch: unknown form / flags / modes, DERIV on another form than POLY, a dtype other than MDSP_F32 / F64, negative sizes,
 *   chunks < 0, a NULL or non-finite coefficient, nden != 0 for SECTIONS, POLY without a numerator, an output that overlaps the input:
 *   MDSP_ERR_ARGUMENT; more than 16 sections: MDSP_ERR_UNSUPPORTED.  nw == 0 succeeds without a launch.
 *   The coefficients are copied at creation; a plan touches the device at its first exec (allocation and a blocking hipMemcpy: not inside a capture).
 * ---------------------------------------------------------------------------------------------------- */
enum { MDSP_RESP_POLY = 0, MDSP_RESP_SECTIONS = 1, MDSP_RESP_ZPK = 2 };
enum { MDSP_RESP_DERIV = 1, MDSP_RESP_NEG = 2 };
enum { MDSP_RESP_COMPLEX = 0, MDSP_RESP_ANGLE = 1, MDSP_RESP_REAL_MINUS = 2 };
enum { MDSP_RESP_W = 0, MDSP_RESP_POINTS = 1 };
typedef struct mdsp_resp_plan_s* mdsp_resp_plan;
int mdsp_resp_plan_create(mdsp_resp_plan* plan, int form, int flags, int out_mode, int in_mode, int dtype, const double* num, int64_t nnum,
                          const double* den, int64_t nden, double gain, double cminus, int64_t nw, int64_t chunks);
int mdsp_resp_plan_destroy(mdsp_resp_plan plan);
int mdsp_resp_plan_info(mdsp_resp_plan plan, int64_t* nchunks, int64_t* chunk_len, int64_t* workspace_bytes);
int mdsp_resp_exec(mdsp_resp_plan plan, const void* w_or_points_dev, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed; ncoef: the longer of the two coefficient vectors.  Any output pointer may be NULL. */
int mdsp_resp_geometry_for(int form, int dtype, int64_t ncoef, int has_den, int64_t nw, int64_t chunks, int64_t* nchunks, int64_t* chunk_len,
                           int64_t* workspace_bytes);
/* Host emulation of the device code (no device): the same cut, chunk order, squaring chain and operators (csrc/resp_op.h) on host arrays, POINTS input. */
int mdsp_resp_emulate_host(const void* points_host, void* out_host, int form, int flags, int out_mode, int dtype, const double* num, int64_t nnum,
                           const double* den, int64_t nden, double gain, double cminus, int64_t nw, int64_t chunks);

/* ------------------------------------------------------------------------------------------------------
 * Deterministic reductions along one dimension (rms, rmsfft, meanfreq, finddelay of src/util.jl:186-220, :336-347).  The array is
 *   (inner, len, outer) as for unwrap, reduced along len; one result per line, line = i + inner o:
 *     MDSP_REDUCE_SUMABS2    sum |x|^2; MDSP_F32 / F64 / C32 / C64; result one Float64.  Float32 terms are formed in Float64 (exact products),
 *                            Float64 terms rounded as abs2 (re*re + im*im, no FMA contraction).
 *     MDSP_REDUCE_SUMABS2_W  complex bins X_k, k = 0 .. len-1: result two Float64, sum p_k (k step) and sum p_k, with p_k = abs2(X_k)
 *                            rounded in the element's real type; `step` = fs / len.  No |X|^2 array is written.
 *     MDSP_REDUCE_ABSARGMAX  a real line and `centre` >= 0: result two Int64, (index, flag).  The larger |x| wins; at equal |x| the index
 *                            nearer to centre; at equal distance the smaller index.  NaN samples do not compete and set flag = 1; a line
 *                            without a candidate gives index -1.
 *   Store, then sum: no atomics, nothing waits for another workgroup; every addition is one Float64 add in the order csrc/reduce_op.h
 *   defines, so one plan gives the same bits exec after exec and equals the host emulation bit for bit.  `depth` bounds the additions any
 *   term passes through.  inner == 1: contiguous route (16-byte loads, ragged head and tail by element: any element alignment); inner > 1:
 *   strided route (a lane per inner index).  segments as for unwrap (0 = auto, > 0 forced, clamped to len); S == 1 is one launch, S > 1 two
 *   (partials into the plan's workspace, then a finish).  The order of the contiguous route depends on (address / element size) mod
 *   (16 / element size) of the array -- `phase` of the emulation -- and on nothing else of the address.
 *   Checks before any launch: sizes < 0, unknown op, a dtype the op does not take, segments < 0, centre < 0: MDSP_ERR_ARGUMENT.  inner or
 *   outer == 0 succeeds without a launch; len == 0 gives 0 / index -1.
 * ---------------------------------------------------------------------------------------------------- */
enum { MDSP_REDUCE_SUMABS2 = 0, MDSP_REDUCE_SUMABS2_W = 1, MDSP_REDUCE_ABSARGMAX = 2 };
enum { MDSP_REDUCE_CONTIGUOUS = 0, MDSP_REDUCE_STRIDED = 1 };
typedef struct mdsp_reduce_plan_s* mdsp_reduce_plan;
int mdsp_reduce_plan_create(mdsp_reduce_plan* plan, int64_t inner, int64_t len, int64_t outer, int op, int dtype, double step, int64_t centre,
                            int64_t segments);
int mdsp_reduce_plan_destroy(mdsp_reduce_plan plan);
int mdsp_reduce_plan_info(mdsp_reduce_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* depth, int64_t* workspace_bytes);
/* out_dev: 8 bytes (SUMABS2) or 16 bytes (the other two) per line, 8-byte aligned. */
int mdsp_reduce_exec(mdsp_reduce_plan plan, const void* in_dev, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_reduce_geometry_for(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, int* route, int64_t* nsegments,
                             int64_t* seglen, int64_t* depth, int64_t* workspace_bytes);
/* Host emulation of the device code (no device): the same geometry, operators and lane walks on host arrays.  depth_reached (may be NULL):
 * the longest chain of additions the run went through. */
int mdsp_reduce_emulate(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int op, int dtype, double step,
                        int64_t centre, int64_t segments, int64_t phase, int64_t* depth_reached);

/* ------------------------------------------------------------------------------------------------------
 * jacobsen and quinn (src/estimation.jl:93-220): the frequency of the largest sinusoid in a vector (csrc/estimation.hip).
 *
 * Reductions (csrc/est_op.h: operators for the templates, the cut and the order of additions of the reductions above; the operator numbers of
 * mdsp_reduce_* are not extended).  Arguments, routes, segments, phase and depth as for mdsp_reduce_*:
 *     MDSP_EST_SUM          the Float64 sum of a line, every element converted exactly; MDSP_F32 / F64: one Float64, MDSP_C32 / C64: two (re, im).
 *     MDSP_EST_ABS2ARGMAX   complex bins X_k: two Int64, (index, flag).  The largest |X_k|^2 -- formed in Float64 as SUMABS2 forms it -- wins, at
 *                           equal value the smaller index (findmax's first maximum).  A bin whose |X|^2 is NaN does not compete and sets flag = 1;
 *                           a line without a candidate gives index -1.
 *   mdsp_est_peak_gather: from the bins of one transform of n >= 2 samples (onesided: nbins = n / 2 + 1 bins, else nbins = n) and an ABS2ARGMAX result,
 *   one record of eight 8-byte words {index, flag, X[k-1], X[k], X[k+1]} (the bins as (re, im) in Float64), with the reference's wrap-around
 *   (estimation.jl:98-103) for a full transform and the Hermitian mirror at the ends of a one-sided one (X[-1] = conj(X[1]); beyond the last bin
 *   X[k+1] = conj(X[n-k-1])).  index -1: the bins are written as zeros.  One launch of one lane; mdsp_est_peak_emulate runs the same text on host arrays.
 *
 * quinn: one PASS of the iteration is a linear recurrence over the signal whose result is a record of a few sums; the filtered signal is never
 * stored.  State and arithmetic are Float64 for every dtype; the mean is removed at the load, d_t = (double)x_t - mean, one rounding.
 *     MDSP_F32 / F64 (Quinn & Fernandes, :175-182), param = alpha:  xi_t = d_t + fma(alpha, xi_(t-1), -xi_(t-2)) from a zero state (at t = 2 one
 *         rounding more than the reference's muladd); record of four doubles {sum_(t=3..n) (xi_t + xi_(t-2)) xi_(t-1), sum_(t=1..n-1) xi_t^2, xi_1, xi_2}.
 *     MDSP_C32 / C64 (Quinn, :205-212), param = omega:  xi_t = d_t + cis(omega) xi_(t-1); record of three doubles
 *         {re S, im S, sum_(t=1..n-1) |xi_t|^2}, S = sum_(t=2..n) d_t conj(xi_(t-1)).
 *   Given the state at its first sample every run of 16 samples is computed by exactly that serial recurrence; a scan with powers of the
 *   recurrence's matrix (host, long double, rounded once, passed in the kernel arguments: no copy per iteration) supplies the start states
 *   (csrc/quinn_scan.h, which also fixes every rounding and the order of every addition).  segments as for mdsp_sos_*: 0 = automatic, > 0 forced
 *   (ceil(n / segments) samples each, clamped to n); S == 1 is one launch, S > 1 four (end states, carries, sums, finish) with 32 (complex: 40) bytes of
 *   workspace per segment.  tile = 64 run samples.  No atomics, nothing waits: a record depends on the arguments only and equals
 *   mdsp_quinn_pass_emulate_host bit for bit.  mean: two doubles (re, im; im ignored for a real dtype).
 *   mdsp_quinn_estimate is the whole algorithm: the mean (one MDSP_EST_SUM reduction), then the reference's iteration and stopping rule; per iteration
 *   one pass, one copy of the record and one synchronisation of `stream`.  estimate in Hz, reached_maxiters as the reference's second result,
 *   iterations (may be NULL) the passes run.  A parameter that is not finite gives a NaN record without a launch, so a NaN runs to maxiters and returns
 *   (NaN, 1) as in the reference.
 *   Checks, before any launch: a bad dtype, n < 2, segments < 0, NULL or misaligned buffers: MDSP_ERR_ARGUMENT.  Powers that are not finite in
 *   Float64 (an iterate with |alpha| > 2 on a long signal): MDSP_ERR_UNSUPPORTED.  A final |beta| > 2 (the reference's acos throws): MDSP_ERR_DOMAIN.
 *   A plan touches the device at its first exec (allocations: not inside a stream capture); mdsp_quinn_estimate synchronises and cannot be captured.
 * ---------------------------------------------------------------------------------------------------- */
enum { MDSP_EST_SUM = 0, MDSP_EST_ABS2ARGMAX = 1 };
typedef struct mdsp_est_reduce_plan_s* mdsp_est_reduce_plan;
int mdsp_est_reduce_plan_create(mdsp_est_reduce_plan* plan, int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments);
int mdsp_est_reduce_plan_destroy(mdsp_est_reduce_plan plan);
int mdsp_est_reduce_plan_info(mdsp_est_reduce_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* depth, int64_t* workspace_bytes);
/* out_dev: 8 bytes (SUM of a real line) or 16 bytes per line, 8-byte aligned. */
int mdsp_est_reduce_exec(mdsp_est_reduce_plan plan, const void* in_dev, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_est_reduce_geometry_for(int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments, int* route, int64_t* nsegments,
                                 int64_t* seglen, int64_t* depth, int64_t* workspace_bytes);
/* Host emulation of the device code (no device). */
int mdsp_est_reduce_emulate(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int op, int dtype, int64_t segments,
                            int64_t phase, int64_t* depth_reached);
/* dtype: MDSP_C32 / C64 of the bins; argmax: the two Int64 of an ABS2ARGMAX result; out: 64 bytes, 8-byte aligned. */
int mdsp_est_peak_gather(const void* bins_dev, int64_t nbins, int64_t n, int onesided, int dtype, const void* argmax_dev, void* out_dev, void* stream);
int mdsp_est_peak_emulate(const void* bins_host, int64_t nbins, int64_t n, int onesided, int dtype, const void* argmax_host, void* out_host);

typedef struct mdsp_quinn_plan_s* mdsp_quinn_plan;
int mdsp_quinn_plan_create(mdsp_quinn_plan* plan, int dtype, int64_t n, int64_t segments);
int mdsp_quinn_plan_destroy(mdsp_quinn_plan plan);
int mdsp_quinn_plan_info(mdsp_quinn_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run, int64_t* workspace_bytes);
/* One pass.  out_dev: four doubles (real dtype) or three (complex), 8-byte aligned. */
int mdsp_quinn_pass_exec(mdsp_quinn_plan plan, const void* x_dev, const double* mean, double param, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_quinn_geometry_for(int dtype, int64_t n, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run,
                            int64_t* workspace_bytes);
/* Host emulation of one pass (no device): the same cut, tiles, scan order, arithmetic and order of additions (csrc/quinn_scan.h) on a host array. */
int mdsp_quinn_pass_emulate_host(const void* x_host, int dtype, int64_t n, int64_t segments, const double* mean, double param, double* out_host);
int mdsp_quinn_estimate(mdsp_quinn_plan plan, const void* x_dev, double f0, double fs, double tol, int64_t maxiters, double* estimate,
                        int* reached_maxiters, int64_t* iterations, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * arburg / lpc(x, p, LPCBurg()) (src/lpc.jl:28-32, :53-92): Burg's method on one vector of n samples of dtype F (R its real type), as p lattice
 *   passes over two work arrays of n elements of F that the plan owns (csrc/lpc.hip, csrc/burg_op.h).  Neither array moves: at order m
 *   element i of ef pairs with element i + m of eb.  On one stream, without a host round trip: a pass over x that leaves the partials of dot(x, x) and
 *   of the order-1 inner product; then for m = 1 .. p a finish (one wavefront: folds the partials in a fixed order, adds the products at the segment
 *   boundaries, takes the scalar step in F / R) and, for m < p, a sweep (the element-wise update fused with the partials of the order-(m+1) inner
 *   product).  2 p launches (p = 0: two).  The partial sums are Float64, stored and summed in a fixed order: no atomics, nothing waits, and a record
 *   depends on (x, p, the cut) only and equals mdsp_burg_emulate_host bit for bit.  x is never written.
 *   The record: 2 p + 2 elements of F -- a[0 .. p] (a[0] = 1), the p reflection coefficients, prediction_err in the real part of the last element
 *   (complex F: its imaginary part is 0).  record_dev is aligned to sizeof(F).
 *   segments: 0 = automatic, > 0 forced: the cut of the pair range [0, n - 1) into ceil((n - 1) / segments) pairs each, fixed for all orders.
 *   tile = 64 x (16 / sizeof(F)) pairs.  workspace_bytes: the two arrays, 24 bytes per segment, the state.
 *   Checks, before any launch: a bad dtype, n < 1, segments < 0, p < 0 or p > n - 1, NULL or misaligned buffers: MDSP_ERR_ARGUMENT.  (The reference
 *   accepts p = n and divides zero by zero there.)  A plan touches the device at its first exec (allocations: not inside a stream capture).
 *   The work arrays, the partials and the state belong to the PLAN: one exec of a plan at a time.  Calls on one stream are ordered by the stream;
 *   two streams (or two threads) that run the same plan at once would interleave on its work arrays -- give each its own plan.  (The Python host
 *   keeps one plan per thread context, dtype and n and always launches on the current stream.)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_burg_plan_s* mdsp_burg_plan;
int mdsp_burg_plan_create(mdsp_burg_plan* plan, int dtype, int64_t n, int64_t segments);
int mdsp_burg_plan_destroy(mdsp_burg_plan plan);
int mdsp_burg_plan_info(mdsp_burg_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* workspace_bytes);
int mdsp_burg_exec(mdsp_burg_plan plan, const void* x_dev, int64_t p, void* record_dev, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_burg_geometry_for(int dtype, int64_t n, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* workspace_bytes);
/* Host emulation of the whole recursion (no device): the same cut, tiles, arithmetic and order of additions (csrc/burg_op.h) on a host array. */
int mdsp_burg_emulate_host(const void* x_host, int dtype, int64_t n, int64_t segments, int64_t p, void* record_host);

/* ------------------------------------------------------------------------------------------------------
 * The Gram matrix of esprit's Hankel matrix (src/estimation.jl:69-71): for one vector of n samples of dtype F, X[i, k] = x[i + k] with M rows and
 *   L = n - M + 1 columns, R = X X^H (csrc/gram.hip, csrc/gram_op.h).  The first p left singular vectors of X span the dominant
 *   p-dimensional eigenspace of R, which is all esprit uses of the SVD; the hosts finish with an M x M Hermitian eigenproblem.
 *   R: M x M, column-major with leading dimension ldr >= M, Float64 for a real F and ComplexF64 for a complex one; aligned to 8 bytes.  Exactly
 *   Hermitian (the upper triangle is stored as the conjugate of the lower), the diagonal's imaginary part +0.0.  Rows M .. ldr - 1 are not touched.
 *   R[j + d, j] is a window sum of x[k + d] conj(x[k]) over L values of k: the body k = M - 1 .. L - 1 that all windows of a diagonal share (one
 *   pass over the signal for all M lags: a partial per (segment, lag), stored, then summed in segment order) plus a head and a tail of at most
 *   M - 1 products each (one lane per diagonal, two running sums); never a difference of running totals.  Products and sums in Float64.  Two
 *   launches on one stream.  No atomics, nothing waits: R depends on (x, M, the cut) only and equals mdsp_hankel_gram_emulate_host bit for bit.
 *   x is never written.
 *   segments: 0 = automatic, > 0 forced: the cut of the body range into ceil((n - 2 M + 2) / segments) samples each.  tile: samples a workgroup
 *   stages at a time; lag_group: lags a lane accumulates at a time.  workspace_bytes: nsegments x M partials of 8 (real) or 16 bytes.
 *   Checks, before any launch: a bad dtype, n < 0, M < 1, segments < 0, ldr < M, NULL or misaligned buffers: MDSP_ERR_ARGUMENT.  2 M - 1 > n (the
 *   windows would share no body; the transposed Hankel matrix has the same row space question turned round) or M > 2^20: MDSP_ERR_UNSUPPORTED.
 *   A plan touches the device at its first exec (allocations: not inside a stream capture); the partials belong to the PLAN: one exec at a time.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_hankel_gram_plan_s* mdsp_hankel_gram_plan;
int mdsp_hankel_gram_plan_create(mdsp_hankel_gram_plan* plan, int dtype, int64_t n, int64_t M, int64_t segments);
int mdsp_hankel_gram_plan_destroy(mdsp_hankel_gram_plan plan);
int mdsp_hankel_gram_plan_info(mdsp_hankel_gram_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* lag_group,
                               int64_t* workspace_bytes);
int mdsp_hankel_gram_exec(mdsp_hankel_gram_plan plan, const void* x_dev, void* r_dev, int64_t ldr, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_hankel_gram_geometry_for(int dtype, int64_t n, int64_t M, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile,
                                  int64_t* lag_group, int64_t* workspace_bytes);
/* Host emulation (no device): the same cut, tiles, arithmetic and order of additions (csrc/gram_op.h) on a host array. */
int mdsp_hankel_gram_emulate_host(const void* x_host, int dtype, int64_t n, int64_t M, int64_t segments, void* r_host, int64_t ldr);

/* ------------------------------------------------------------------------------------------------------
 * shiftsignal / shiftsignal! (src/util.jl:357-395): y[i] = x[i - s] where that exists, else 0, one line of l elements of 4, 8 or 16 bytes
 *   (moved as words: any element type).  in_place: out is the input.  Routes, chosen at plan creation and reported:
 *     MDSP_SHIFT_DISJOINT  out of place, or in place with 2 |s| >= l; one launch
 *     MDSP_SHIFT_HALO      in place, 0 < |s| < l / 2: destination tiles of max(tile, |s|) elements, their halos copied to the workspace
 *                          first (|s| elements per tile), then a workgroup per tile walking chunks towards its sources; two launches
 *     MDSP_SHIFT_STAGED    HALO would leave fewer than 256 tiles: the source range goes through the workspace (l - |s| elements); two launches
 *   tile: 0 = 256 KiB of elements, > 0 forced (tests); route: MDSP_SHIFT_AUTO or a forced route -- DISJOINT where source and destination
 *   overlap, or HALO out of place or with s == 0, is MDSP_ERR_ARGUMENT.  |s| > l: MDSP_ERR_DOMAIN.  In place with s == 0 and l == 0 succeed
 *   without a launch.  Why each route is safe in place: csrc/shift_plan.h, DESIGN.md section 4.12.
 * ---------------------------------------------------------------------------------------------------- */
enum { MDSP_SHIFT_AUTO = 0, MDSP_SHIFT_DISJOINT = 1, MDSP_SHIFT_HALO = 2, MDSP_SHIFT_STAGED = 3 };
typedef struct mdsp_shift_plan_s* mdsp_shift_plan;
int mdsp_shift_plan_create(mdsp_shift_plan* plan, int64_t l, int64_t s, int64_t elem_bytes, int in_place, int64_t tile, int route);
int mdsp_shift_plan_destroy(mdsp_shift_plan plan);
int mdsp_shift_plan_info(mdsp_shift_plan plan, int* route, int64_t* tile, int64_t* chunk, int64_t* ntiles, int64_t* workspace_bytes);
/* out_dev == in_dev exactly when the plan was made in place; any other overlap is MDSP_ERR_ARGUMENT. */
int mdsp_shift_exec(mdsp_shift_plan plan, const void* in_dev, void* out_dev, void* stream);
/* Pure host arithmetic, no device needed.  Any output pointer may be NULL. */
int mdsp_shift_geometry_for(int64_t l, int64_t s, int64_t elem_bytes, int in_place, int64_t tile, int route, int* route_out, int64_t* tile_out,
                            int64_t* chunk, int64_t* ntiles, int64_t* workspace_bytes);
/* Host emulation (no device) of the plan's launches, the units of a launch in the order `order` (0 ascending, 1 descending, 2 odd ones
 * first); out_host == in_host is in place.  violations (may be NULL): reads of a word of the line after it was written, and HALO reads of a
 * word outside the reader's own tile -- 0 for a correct schedule. */
int mdsp_shift_emulate(const void* in_host, void* out_host, int64_t l, int64_t s, int64_t elem_bytes, int64_t tile, int route, int order,
                       int64_t* violations);

/* ------------------------------------------------------------------------------------------------------
 * Multitaper spectral estimation (src/multitaper.jl)
 *   plan    = MTConfig (:5-135): frames of n samples, nfft, `ntapers` tapers (n x ntapers, column-major Float64,
 *             e.g. dpss(n, nw, ntapers)), inverse normalisations r[taper] (fs ./ taper_weights, :127-131)
 *   psd     = mt_pgram! (:225-245) for every frame of arraysplit(signal, n, noverlap): mt_spectrogram! (:312-330);
 *             out: (nout, K) per channel, like mdsp_stft_exec with psd_only
 *   spectra = mt_fft_tapered_multichannel! (:596-600): x_mt[f, taper, channel] of ONE n-sample frame per channel
 *             (real input, onesided), optionally demeaned per channel (:566-570)
 *   cross   = cs_inner! (:602-616) incl. the DC / Nyquist 1/sqrt(2) (:577-580): out (nch, nch, nfi) complex
 *   coherence_from_cs! (:704-723): (nch, nch, nf) complex -> real
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_mt_plan_s* mdsp_mt_plan;
int mdsp_mt_plan_create(mdsp_mt_plan* plan, int64_t n, int64_t nfft, const double* tapers_host, int64_t ntapers,
                        const double* r_host, int onesided, int dtype, int engine);
int mdsp_mt_plan_destroy(mdsp_mt_plan plan);
int mdsp_mt_plan_info(mdsp_mt_plan plan, int64_t* nout, int64_t* ntapers, int* engine_used);
int mdsp_mt_psd_exec(mdsp_mt_plan plan, const void* s_dev, int64_t len, int64_t noverlap, int64_t nch, int64_t lds,
                     void* out_dev, int64_t ldo, int64_t chs, void* stream);
int mdsp_mt_spectra_exec(mdsp_mt_plan plan, const void* s_dev, int64_t nch, int64_t lds, int demean, void* xmt_dev,
                         void* stream);
int mdsp_mt_cross_spectra(mdsp_mt_plan plan, const void* xmt_dev, int64_t nch, const int64_t* freq_inds_host /*0-based*/,
                          int64_t nfi, void* out_dev, void* stream);
int mdsp_coherence_from_cs(const void* cs_dev, int64_t nch, int64_t nf, int real_dtype, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Stateful polyphase FIR (FIRFilter{FIRStandard|FIRInterpolator|FIRDecimator|FIRRational})
 *   replaces the while loop of filt!(buffer, ::FIRFilter, x) (stream_filt.jl:409-558) and its
 *   unsafe_dot / BLAS.dot inner products (util.jl:225-283) and shiftin! (util.jl:299-314).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_fir_s* mdsp_fir;
/* taps_host: hlen taps of taps_dtype (MDSP_F32 | MDSP_F64 | MDSP_C32 | MDSP_C64; complex taps as interleaved (re, im) pairs, multiplied
 * as they are: no conjugate); ratio L/M is reduced to lowest terms.
 * x_dtype: element type of the input; output type = promote(taps, x) -- complex when either is, double when either is.  nch channels share the scalar state
 * (phi_idx, input_deficit) and keep separate histories, as resample(...; dims) does per slice (:768-774). */
int mdsp_fir_create(mdsp_fir* f, const void* taps_host, int64_t hlen, int64_t L, int64_t M, int taps_dtype,
                    int x_dtype, int64_t nch);
int mdsp_fir_destroy(mdsp_fir f);
/* exact != 0: this filter runs the generic kernel only, in which every output reads exactly its own tapsPerPhi-sample window
 * (stream_filt.jl:496-509) -- a NaN / Inf sample then leaves exactly the reference's hole.  The default kernels multiply a tile's common window
 * by explicit zero taps, so their hole can be wider by up to 15 outputs plus the outputs of 64 more input positions (the decimator kernel, L = 1,
 * is exact either way).  Same results otherwise, to rounding.  (Round 4 had this as the process-wide environment variable MDSP_FIR_EXACT only.) */
int mdsp_fir_set_exact(mdsp_fir f, int exact);
int mdsp_fir_reset(mdsp_fir f);                       /* reset!     stream_filt.jl:247-276 */
int mdsp_fir_setphase(mdsp_fir f, double phi);        /* setphase!  :216-229 */
int mdsp_fir_timedelay(mdsp_fir f, double* tau);      /* timedelay  :400-403 */
int mdsp_fir_outputlength(mdsp_fir f, int64_t inputlength, int64_t* outlen);            /* :324-338 */
int mdsp_fir_inputlength(mdsp_fir f, int64_t outputlength, int round_up, int64_t* inlen); /* :366-383 */
int mdsp_fir_info(mdsp_fir f, int* kind /*0 std,1 interp,2 decim,3 rational*/, int64_t* L, int64_t* M,
                  int64_t* taps_per_phase, int64_t* history_len, int* out_dtype);
/* Which kernel mdsp_fir_exec would run for a chunk of `xlen` samples in the filter's current state: 0 generic polyphase kernel
 * (any dtype), 1 register-tap kernel (Float32 <= 64 taps per phase; Float64 / ComplexF32 / ComplexF64 <= 112, L <= 1024), 2 matrix-core kernel (rows of 16 outputs on
 * v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64; Float32 results bit-identical to 0 / 1), 3 decimator kernel (L = 1, M <= 64, any length: a lane
 * per input phase; sums phases first, so it agrees with 0 to rounding, and reads exactly the reference's windows).  Complex taps: 1 the complex
 * register-tap kernel (Float32 arithmetic <= 112 taps per phase, Float64 <= 56, L <= 1024), 0 the generic kernel; never 2 or 3.  Diagnostics / tests. */
int mdsp_fir_kernel_path(mdsp_fir f, int64_t xlen, int* path);
/* Geometry the matrix-core kernel would use for a filter of hlen taps at ratio L // M (pure host arithmetic, no device):
 * out12 = {fits, rounds per row RB, outputs per row Lr = RB L, samples per row Mr = RB M, column blocks NB, row groups NG, k-steps of four taps (in registers up to 64, Float64 32; beyond that fetched per tile),
 * 16-row chunks per wave CH, parts per sample CS, DMA waves, store waves, LDS bytes}.  fits = 0 for complex taps.  Diagnostics / tests. */
int mdsp_fir_mm_geometry(int64_t L, int64_t M, int64_t hlen, int taps_dtype, int x_dtype, int64_t* out12);
/* state is exactly the reference's: 1-based phi_idx and input_deficit, history (history_len, nch) of x_dtype */
int mdsp_fir_get_state(mdsp_fir f, int64_t* phi_idx, int64_t* input_deficit, void* history_host);
int mdsp_fir_set_state(mdsp_fir f, int64_t phi_idx, int64_t input_deficit, const void* history_host);
/* x_dev: (xlen, nch) ld ldx;  y_dev: (ycap, nch) ld ldy, ycap >= outputlength (ArgumentError otherwise, :490).
 * *nwritten = samples written per channel (the return value of filt!). */
int mdsp_fir_exec(mdsp_fir f, const void* x_dev, int64_t xlen, int64_t ldx, void* y_dev, int64_t ycap,
                  int64_t ldy, int64_t* nwritten, void* stream);
/* filt(::FIRFilter, x) / resample of host arrays (stream_filt.jl:627-637, :688-775): the stream passes through the filter in time chunks of
 * all channels, the filter state carried from chunk to chunk exactly as in the reference's streaming use -- the result and the final state
 * are those of ONE mdsp_fir_exec over the whole stream, bit for bit.  ycap >= mdsp_fir_outputlength(f, xlen).  flags: MDSP_HOST_PINNED */
int mdsp_fir_exec_host(mdsp_fir f, const void* x_host, int64_t xlen, int64_t ldx, void* y_host, int64_t ycap,
                       int64_t ldy, int64_t* nwritten, int flags);

/* ------------------------------------------------------------------------------------------------------
 * Arbitrary-rate resampler (FIRFilter{FIRArbitrary}: rate::AbstractFloat, Nphi phases, linear interpolation
 * between neighbouring phases through the derivative bank)
 *   replaces FIRArbitrary / FIRFilter(h, rate, Nphi) (stream_filt.jl:92-156), update! (:567-577) and
 *   filt!(buffer, ::FIRFilter{FIRArbitrary}, x) (:579-625).  The Float64 phase-accumulator recurrence is evaluated
 *   with the reference's own IEEE operations (host, once per call, shared by all channels), so the number of
 *   samples written and the state after every chunk are bit-exact; the dot products run on the device.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mdsp_firarb_s* mdsp_firarb;
/* taps_dtype: MDSP_F32 | MDSP_F64 (complex taps: MDSP_ERR_UNSUPPORTED -- they run at integer and rational ratios, mdsp_fir_create) */
int mdsp_firarb_create(mdsp_firarb* f, const void* taps_host, int64_t hlen, double rate, int64_t nphi, int taps_dtype,
                       int x_dtype, int64_t nch);
int mdsp_firarb_destroy(mdsp_firarb f);
int mdsp_firarb_reset(mdsp_firarb f);                     /* reset!      stream_filt.jl:260-276 */
int mdsp_firarb_setphase(mdsp_firarb f, double phi);      /* setphase!   :231-239 */
int mdsp_firarb_timedelay(mdsp_firarb f, double* tau);    /* timedelay   :400-401 */
int mdsp_firarb_outputlength(mdsp_firarb f, int64_t inputlength, int64_t* outlen);              /* :340-342 */
int mdsp_firarb_inputlength(mdsp_firarb f, int64_t outputlength, int round_up, int64_t* inlen); /* :385-389 */
int mdsp_firarb_info(mdsp_firarb f, int64_t* nphi, int64_t* taps_per_phase, int64_t* history_len, int* out_dtype,
                     double* delta);
/* the reference's state: phiAccumulator, alpha = frac(phiAccumulator), phiIdx = 1 + trunc(phiAccumulator) (1-based),
 * inputDeficit, xIdx (1-based), history (history_len, nch) of x_dtype */
int mdsp_firarb_get_state(mdsp_firarb f, double* phi_acc, double* alpha, int64_t* phi_idx, int64_t* input_deficit,
                          int64_t* x_idx, void* history_host);
int mdsp_firarb_set_state(mdsp_firarb f, double phi_acc, int64_t input_deficit, const void* history_host);
/* y_dev: (ycap, nch); ycap must hold every sample the loop writes (outputlength(...) + 1 always suffices, which is
 * what allocate_output reserves, :639-655).  *nwritten = samplesWritten. */
int mdsp_firarb_exec(mdsp_firarb f, const void* x_dev, int64_t xlen, int64_t ldx, void* y_dev, int64_t ycap,
                     int64_t ldy, int64_t* nwritten, void* stream);
/* Pure host function (no device): the index trajectory of the loop above.  Writes the (xIdx, phiAccumulator) of
 * outputs 0, block, 2*block, ... into anchors_* (may be NULL), the number of outputs and the final state. */
int mdsp_arb_trajectory(double phi_acc, int64_t input_deficit, double rate, int64_t nphi, int64_t xlen, int64_t block,
                        int64_t* anchors_x, double* anchors_acc, int64_t anchors_cap, int64_t* nout,
                        double* phi_acc_end, int64_t* input_deficit_end);
/* For streams of >= 2^19 outputs mdsp_firarb_exec evaluates that same recurrence in parallel on the device, bit for bit
 * (integer image of the IEEE operations + a multi-level scan of the rounding, dsp.jl_amd/csrc/arb_scan.h), after a
 * serial pilot of `pilot` outputs; it falls back to the serial loop when its self-check cannot certify the result.
 * mdsp_arb_trajectory_scan is the host emulation of that device code (anchors every 16 outputs; *used = 0: the scan
 * does not apply to these arguments); mdsp_firarb_scan_stats counts how each trajectory of a filter was evaluated. */
int mdsp_arb_trajectory_scan(double phi_acc, int64_t input_deficit, double rate, int64_t nphi, int64_t xlen, int64_t pilot,
                             int64_t* anchors_x, double* anchors_acc, int64_t anchors_cap, int64_t* nout,
                             double* phi_acc_end, int64_t* input_deficit_end, int* used, int* passes);
int mdsp_firarb_scan_stats(mdsp_firarb f, int64_t* scanned, int64_t* serial);
/* test helper (host): updates at which the device replay's branch-free form of update! differs from the reference form */
int mdsp_arb_replay_check(double phi_acc, double rate, int64_t nphi, int64_t nsteps, int64_t* mismatches);
/* The launch geometry mdsp_firarb_exec uses for a filter of taps_per_phase x nphi taps at `rate`, nch channels and a chunk of nout outputs:
 * the very host function the launch calls, so what it reports is what runs.  out8 = {tile (outputs per workgroup), span (staged samples per
 * tile and channel; 0: windows read straight from memory), nchg (channels per group: the 4 / 2 / 1 instantiation), groups = ceil(nch / nchg),
 * tiles = ceil(nout / tile), gy (grid rows; gy < groups: each workgroup loops over several channel groups), taps_in_lds (0: tap pairs read from
 * global memory, above 32 KiB of pairs), lds_bytes (dynamic LDS per workgroup)}.  Honours the MDSP_ARB_TILE / MDSP_ARB_NCH knobs.
 * cu_count <= 0: the current device's compute units; with cu_count > 0 it is pure host arithmetic (no device).  Diagnostics / tests. */
int mdsp_arb_kernel_geometry(int64_t taps_per_phase, int64_t nphi, double rate, int taps_dtype, int x_dtype, int64_t nch,
                             int64_t nout, int cu_count, int64_t out8[8]);

/* ------------------------------------------------------------------------------------------------------
 * N-dimensional convolution: conv(u, v) / conv!(out, u, v) for arrays (dspbase.jl:709-792).
 *   u_dev / v_dev: column-major arrays (first dimension fastest) of sizes su[ndim] / sv[ndim], both of `dtype`;
 *   out_dev: column-major, sizes su[d] + sv[d] - 1.
 *   mdsp_convnd_fft    replaces _conv_kern_fft! (dspbase.jl:611-644): per-dimension zero-padding to
 *                      nextfastfft(outsize), one N-d transform per operand (real transforms for real dtypes),
 *                      product, inverse, crop -- and stands in for unsafe_conv_kern_os! (:490-609), which evaluates
 *                      the same sums block-wise.  At most three dimensions with extent > 1 (rocFFT).
 *   mdsp_convnd_direct replaces _conv_td! (dspbase.jl:646-660): the convolution sum, any ndim <= 8.
 * ---------------------------------------------------------------------------------------------------- */
int mdsp_convnd_fft(const void* u_dev, const int64_t* su, const void* v_dev, const int64_t* sv, int ndim, int dtype,
                    void* out_dev, void* stream);
int mdsp_convnd_direct(const void* u_dev, const int64_t* su, const void* v_dev, const int64_t* sv, int ndim, int dtype,
                       void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Time-domain FIR (filt(b, a::Number, x) and the nb <= 66 branch of filt(b, x)):
 *   replaces _filt_fir! (dspbase.jl:95-105,118-141).  Zero initial state, per column.
 *   taps_host: nb REAL taps in the real precision of `dtype` (float for MDSP_F32/C32, double for F64/C64);
 *   x_dev / y_dev: (nx, ncols) of `dtype`.
 * ---------------------------------------------------------------------------------------------------- */
int mdsp_tdfir_exec(const void* taps_host, int64_t nb, int dtype, const void* x_dev, int64_t nx, int64_t ncols,
                    int64_t ldx, void* y_dev, int64_t ldy, void* stream);
/* The same with an explicit tap dtype: taps_host holds nb taps of taps_dtype (any of the four; complex taps are multiplied as they are, no
 *   conjugate), x_dev is (nx, ncols) of x_dtype and y_dev of promote(taps_dtype, x_dtype). */
int mdsp_tdfir_exec_t(const void* taps_host, int64_t nb, int taps_dtype, int x_dtype, const void* x_dev, int64_t nx,
                      int64_t ncols, int64_t ldx, void* y_dev, int64_t ldy, void* stream);

/* Stateful time-domain FIR: filt!(out, f::DF2TFilter{<:PolynomialRatio}, x) with FIR coefficients (Filters/filt.jl:153-181)
 *   advancing the TDF-II state exactly as _filt_fir!(out, b, x, si, col) does (dspbase.jl:95-105).
 *   si_dev: (nb-1, ncols) of `dtype`, read as the initial state and overwritten with the final one. */
int mdsp_tdfir_state_exec(const void* taps_host, int64_t nb, int dtype, const void* x_dev, int64_t nx, int64_t ncols,
                          int64_t ldx, void* y_dev, int64_t ldy, void* si_dev, void* stream);
/* The same with an explicit tap dtype, so that complex coefficients carry a complex TDF-II state (zeros(promote_type(T, V), ...),
 *   Filters/filt.jl:149-151).  The state is of the promoted type and the signal enters the recursion in it, so x_dev, y_dev and si_dev are all of
 *   x_dtype, which must equal promote(taps_dtype, x_dtype) (the caller widens a narrower signal); the taps are in x_dtype's precision, real or complex. */
int mdsp_tdfir_state_exec_t(const void* taps_host, int64_t nb, int taps_dtype, int x_dtype, const void* x_dev, int64_t nx,
                            int64_t ncols, int64_t ldx, void* y_dev, int64_t ldy, void* si_dev, void* stream);
/* extrapolate_signal! (Filters/filt.jl:243-257), the odd-symmetric extension filtfilt applies per column:
 *   out (n + 2 pad, ncols) = [2 x[1] .- x[pad+1:-1:2]; x; 2 x[end] .- x[end-1:-1:end-pad]] */
int mdsp_extrapolate(const void* x_dev, int64_t n, int64_t ncols, int64_t ldx, int dtype, int64_t pad, void* out_dev,
                     int64_t ldo, void* stream);

/* hilbert(x) (src/util.jl:31-87): analytic signal of every real column, out (n, ncols) complex of the same precision */
int mdsp_hilbert(const void* x_dev, int64_t n, int64_t ncols, int64_t ldx, int real_dtype, void* out_dev, int64_t ldo,
                 void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Plan cache inside the library: the per-call fast path for hosts that mirror DSP.jl's function-style entry points one-to-one
 * (filt(b, x), conv(u, v), welch_pgram(s, n, noverlap), stft / spectrogram / periodogram build their FFTW plans on every call;
 * a device plan costs ~1 ms, the call ~45 us).  Same arguments as the matching *_plan_create plus the stream the plan will run on;
 * the key is (device, partition, stream, every argument, CONTENTS of taps / window).  The returned handle is BORROWED: never destroy it.
 * Partitions: the calling OS thread by default; a host whose logical tasks migrate between OS threads (Julia tasks) binds its own id with
 * mdsp_plan_cache_set_context(id != 0) -- thread-local, 0 restores the per-thread default -- and frees that partition with
 * mdsp_plan_cache_release_context(id).  Only requests of the same partition evict from its two lists (user plans / the library's own cached
 * objects, MDSP_PLAN_CACHE_SIZE each), so a handle stays valid until ITS PARTITION has made MDSP_PLAN_CACHE_SIZE further distinct cached requests,
 * with one exception that bounds device memory: above MDSP_PLAN_CACHE_TOTAL entries in the whole cache (environment, default 8 x
 * MDSP_PLAN_CACHE_SIZE) entries of explicit contexts that NO thread has bound at the moment and that have made no request for MDSP_PLAN_CACHE_IDLE
 * (default 64) cache requests are evicted -- a host therefore keeps its context bound for as long as it uses handles borrowed under it; the
 * partition of a live OS thread is never evicted by others (it may be inside a long call on a borrowed handle).
 * The entries of an OS thread that exits are reaped automatically (destroyed at the next cache request of any thread).
 * mdsp_plan_cache_clear() destroys every partition's entries and must not race with other threads' library calls.
 * mdsp_plan_cache_partitions: live partitions and the number of entries reaped so far (exited threads, released contexts, cap evictions).
 * ---------------------------------------------------------------------------------------------------- */
#define MDSP_PLAN_CACHE_SIZE 16
int mdsp_ols_plan_cached(mdsp_ols_plan* plan, const void* taps_host, int64_t nb, int64_t nfft, int64_t nx_hint, int dtype, int mode,
                         int engine, void* stream);
int mdsp_welch_plan_cached(mdsp_welch_plan* plan, int64_t n, int64_t noverlap, int64_t nfft, const double* window_host, double r,
                           int onesided, int dtype, int engine, void* stream);
int mdsp_stft_plan_cached(mdsp_stft_plan* plan, int64_t n, int64_t noverlap, int64_t nfft, const double* window_host, double r,
                          int onesided, int psd_only, int dtype, int engine, void* stream);
int mdsp_plan_cache_stats(int64_t* entries, int64_t* hits, int64_t* misses);
int mdsp_plan_cache_partitions(int64_t* partitions, int64_t* reaped);
int mdsp_plan_cache_set_context(uint64_t id);
int mdsp_plan_cache_release_context(uint64_t id);
int mdsp_plan_cache_clear(void);

/* ------------------------------------------------------------------------------------------------------
 * Measurement helpers (used by bench.py; not part of the drop-in surface)
 * ---------------------------------------------------------------------------------------------------- */
/* Times `reps` back-to-back launches of the last exec recorded on a plan with HIP events on `stream`. */
int mdsp_event_create(void** ev);
int mdsp_event_destroy(void* ev);
int mdsp_event_record(void* ev, void* stream);
int mdsp_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
/* float4 device copy kernel: the on-box achievable-HBM yardstick (bytes read + written = 2*bytes). */
int mdsp_copy_bench(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
/* The same yardstick with an explicit access pattern: mode 0 float4 copy (grid-stride), 1 four float loads/stores, 2 nontemporal float4,
 * 3 one contiguous chunk per workgroup, 4 read-only (float4 loads summed), 5 write-only; wgs = workgroups per CU (< 1: 8). */
int mdsp_copy_bench_mode(void* dst_dev, const void* src_dev, size_t bytes, int mode, int wgs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355DSP_H */
