# MI355DSP.jl -- thin Julia host for libmi355dsp.so (the C ABI of include/mi355dsp.h).
#
# STATUS: written against the header, NOT executed -- the build image has no Julia.  The same C ABI is exercised
# by the Python/ctypes host (dsp.jl_amd/) and its GPU parity tests; this file is the `ccall` twin a DSP.jl
# maintainer would use.  tests/test_abi_cpu.py checks every `ccall` here against the ctypes prototype of the same
# entry point: symbol exported, argument count, and every argument TYPE (Cint / Int64 / Cdouble / Csize_t / pointer kind).
#
# It keeps DSP.jl's names, argument order, defaults, promotion rules, result types (`Periodogram`, `Spectrogram` with
# `power` / `freq` / `time`) and exception types for the hot path -- filt / filt! / fftfilt / fftfilt! / tdfilt / tdfilt! /
# conv / conv! / xcorr / hilbert / periodogram / welch_pgram / welch_pgram! / spectrogram / stft / arraysplit / FIRFilter /
# resample / DF2TFilter / filtfilt / the mt_* family -- and does nothing else: no CUDA.jl / AMDGPU.jl array dispatch, every
# call goes straight to a hand-written HIP kernel through `ccall`.
#
# Host `Array`s go through the library's host-pointer pipelines (mdsp_{ols,welch,stft,fir}_exec_host: H2D || kernel || D2H on
# three streams; `pin!` page-locks an Array so the DMA engines use it directly); `DeviceArray` keeps data resident in HBM
# between calls.  The function-style calls take their plans from the library's own LRU (mdsp_*_plan_cached, one list per
# calling thread); the multi-GPU part is `Comm` (RCCL behind the C ABI).  Reference locations are DSP.jl v0.8.5 `src/`.
module MI355DSP

using LinearAlgebra: Hermitian, SymTridiagonal, eigen

export DeviceArray, upload, download, filt, filt!, fftfilt, fftfilt!, tdfilt, tdfilt!, conv, conv!, xcorr, hilbert,
       Periodogram, Periodogram2, Spectrogram, power, freq, fftshift, arraysplit, periodogram, WelchConfig, welch_pgram, welch_pgram!,
       spectrogram, stft, FIRFilter, resample, resample_filter, reset!, setphase!, timedelay, inputlength, outputlength,
       DF2TFilter, filtfilt, nextfastfft, optimalfftfiltlength, Comm, welch_channel_mean, welch_reset!, welch_accumulate!,
       welch_finalize, welch_allreduce!, pin!, unpin!, MTConfig, mt_pgram, mt_pgram!, MTSpectrogramConfig, mt_spectrogram,
       mt_spectrogram!, MTCrossSpectraConfig, mt_cross_power_spectra, mt_cross_power_spectra!, MTCoherenceConfig,
       mt_coherence, mt_coherence!, CrossPowerSpectra, Coherence, coherence, dpss, unwrap, unwrap!, sosfilt, sosfilt!,
       resp, resp_geometry, resp_emulate, impresp, stepresp,
       rms, rmsfft, meanfreq, finddelay, shiftsignal, shiftsignal!, alignsignals, alignsignals!, pow2db, amp2db, db2pow, db2amp,
       jacobsen, quinn, quinn_geometry, quinn_pass_emulate,
       lpc, arburg, levinson, LPCBurg, LPCLevinson, burg_geometry, burg_emulate,
       esprit, esprit_from_gram, hankel_gram, hankel_gram_geometry, hankel_gram_emulate

const lib = get(ENV, "MI355DSP_LIB", joinpath(@__DIR__, "..", "dsp.jl_amd", "libmi355dsp.so"))

# ---------------------------------------------------------------------------------------------- status -> exception
const MDSP_F32, MDSP_F64, MDSP_C32, MDSP_C64 = Cint(0), Cint(1), Cint(2), Cint(3)
const ENGINE_AUTO, ENGINE_FUSED, ENGINE_ROCFFT = Cint(0), Cint(1), Cint(2)
const OLS_FILT, OLS_CONV = Cint(0), Cint(1)
const HOST_PINNED = Cint(1)

struct UnsupportedError <: Exception
    msg::String
end
struct DeviceError <: Exception
    msg::String
end

lasterr() = unsafe_string(ccall((:mdsp_last_error_string, lib), Cstring, ()))

function check(status::Cint)
    status == 0 && return nothing
    msg = lasterr()
    status == -1 && throw(ArgumentError(msg))          # dspbase.jl:28-33, filt.jl:474,531, periodograms.jl:396,564,876
    status == -2 && throw(DomainError(nothing, msg))   # periodograms.jl:44-45,397,565; stream_filt.jl:194,217
    status == -3 && throw(DimensionMismatch(msg))      # periodograms.jl:255,735-737
    status == -4 && throw(AssertionError(msg))         # stream_filt.jl:634,718,722
    status == -5 && throw(UnsupportedError(msg))       # caller should fall back to DSP.jl itself
    status == -7 && throw(OutOfMemoryError())
    throw(DeviceError(msg))
end

mdtype(::Type{Float32}) = MDSP_F32
mdtype(::Type{Float64}) = MDSP_F64
mdtype(::Type{ComplexF32}) = MDSP_C32
mdtype(::Type{ComplexF64}) = MDSP_C64
const JLTYPE = (Float32, Float64, ComplexF32, ComplexF64)

# element-type rules, util.jl:92-104
fftintype(::Type{T}) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}} = T
fftintype(::Type{T}) where {T<:Real} = Float64
fftintype(::Type{T}) where {T<:Complex} = ComplexF64
fftouttype(::Type{T}) where {T<:Union{ComplexF32,ComplexF64}} = T
fftouttype(::Type{Float32}) = ComplexF32
fftouttype(::Type{T}) where {T<:Union{Real,Complex}} = ComplexF64
fftabs2type(::Type{T}) where {T<:Union{Float32,ComplexF32}} = Float32
fftabs2type(::Type{T}) where {T<:Union{Real,Complex}} = Float64

# ---------------------------------------------------------------------------------------------- library state / diagnostics
init(device::Integer=0) = check(ccall((:mdsp_init, lib), Cint, (Cint,), device))
shutdown() = check(ccall((:mdsp_shutdown, lib), Cint, ()))                         # borrowed plans and staging buffers die here
version() = Int(ccall((:mdsp_version, lib), Cint, ()))
function device_count()
    n = Ref{Cint}(0)
    check(ccall((:mdsp_device_count, lib), Cint, (Ref{Cint},), n)); Int(n[])
end
reload_tunables() = check(ccall((:mdsp_reload_tunables, lib), Cint, ()))           # tuning tools only: re-read the fifteen MDSP_* variables from ENV
set_knob(name::AbstractString, value::Integer) = check(ccall((:mdsp_set_knob, lib), Cint, (Cstring, Cint, Cint), name, value, 0))   # experiments: not environment variables
unset_knob(name::AbstractString) = check(ccall((:mdsp_set_knob, lib), Cint, (Cstring, Cint, Cint), name, 0, 1))
debug_knobs() = ccall((:mdsp_debug_knobs, lib), Cint, ()) != 0
synchronize(stream::Ptr{Cvoid}=C_NULL) = check(ccall((:mdsp_stream_synchronize, lib), Cint, (Ptr{Cvoid},), stream))
function plan_cache_stats()
    e, h, m = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_plan_cache_stats, lib), Cint, (Ref{Int64}, Ref{Int64}, Ref{Int64}), e, h, m))
    (entries = Int(e[]), hits = Int(h[]), misses = Int(m[]))
end
plan_cache_clear() = check(ccall((:mdsp_plan_cache_clear, lib), Cint, ()))
host_pipeline_trim() = check(ccall((:mdsp_host_pipeline_trim, lib), Cint, ()))   # frees the host-array pipelines' device / pinned buffers
function plan_cache_partitions()
    p, r = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_plan_cache_partitions, lib), Cint, (Ref{Int64}, Ref{Int64}), p, r))
    (partitions = Int(p[]), reaped = Int(r[]))
end
# Julia tasks migrate between OS threads, the library's binding is thread-local: `with_plan_context` pins the task to its thread for the duration
# (sticky, restored afterwards), so the binding is made and restored on the SAME thread.  Calls nest: the task keeps a stack of its contexts in
# task-local storage, leaving a level re-binds the level above (not 0), and a context derived from the task (the default id) is released -- its
# plans freed with it -- only when the OUTERMOST level that uses it returns (a nested default-id call derives the same id: releasing it there would
# free plans the outer level still holds).  Pass an id of your own (and call plan_cache_release_context when its work is done) to keep plans across
# calls.  The binding belongs to the OS thread: `f` must not yield to another task that uses the library on this thread without a context of its
# own -- that task would run under this binding while `f` is suspended (wrap it in with_plan_context too: it re-binds on entry and on exit).
plan_cache_set_context(id::Integer) = check(ccall((:mdsp_plan_cache_set_context, lib), Cint, (UInt64,), UInt64(id)))
plan_cache_release_context(id::Integer) = check(ccall((:mdsp_plan_cache_release_context, lib), Cint, (UInt64,), UInt64(id)))
const _CTX_KEY = :mi355dsp_plan_contexts
function with_plan_context(f, id::Union{Integer,Nothing}=nothing)
    t = current_task()
    own = id === nothing
    ctx = own ? (objectid(t) % UInt64) | (UInt64(1) << 62) : UInt64(id)
    stack = get!(() -> UInt64[], task_local_storage(), _CTX_KEY)::Vector{UInt64}
    was_sticky = t.sticky
    t.sticky = true                  # no migration between the bindings below
    push!(stack, ctx)
    plan_cache_set_context(ctx)
    try
        return f()
    finally
        pop!(stack)
        plan_cache_set_context(isempty(stack) ? UInt64(0) : last(stack))   # back to the enclosing level's binding
        own && !(ctx in stack) && plan_cache_release_context(ctx)          # outermost use of the derived context only
        t.sticky = was_sticky
    end
end

# HIP events on the library's launch stream (what bench.py times with)
mutable struct Event
    h::Ptr{Cvoid}
    function Event()
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mdsp_event_create, lib), Cint, (Ref{Ptr{Cvoid}},), p))
        e = new(p[])
        finalizer(x -> ccall((:mdsp_event_destroy, lib), Cint, (Ptr{Cvoid},), x.h), e)
        e
    end
end
record!(e::Event, stream::Ptr{Cvoid}=C_NULL) = (check(ccall((:mdsp_event_record, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), e.h, stream)); e)
function elapsed_ms(a::Event, b::Event)
    ms = Ref{Cfloat}(0)
    check(ccall((:mdsp_event_elapsed_ms, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cfloat}), a.h, b.h, ms)); Float64(ms[])
end

# ---------------------------------------------------------------------------------------------- device memory
mutable struct DeviceArray{T,N}
    ptr::Ptr{Cvoid}
    dims::NTuple{N,Int}
    function DeviceArray{T}(dims::NTuple{N,Int}) where {T,N}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mdsp_malloc, lib), Cint, (Ref{Ptr{Cvoid}}, Csize_t), p, prod(dims) * sizeof(T)))
        a = new{T,N}(p[], dims)
        finalizer(x -> ccall((:mdsp_free, lib), Cint, (Ptr{Cvoid},), x.ptr), a)
        a
    end
end
DeviceArray{T}(dims::Int...) where {T} = DeviceArray{T}(dims)
Base.size(a::DeviceArray) = a.dims
Base.size(a::DeviceArray, d::Integer) = d <= length(a.dims) ? a.dims[d] : 1
Base.length(a::DeviceArray) = prod(a.dims)
Base.eltype(::DeviceArray{T}) where {T} = T
Base.ndims(::DeviceArray{T,N}) where {T,N} = N
function Base.fill!(a::DeviceArray, byte::Integer)          # byte fill (zero the array with 0)
    check(ccall((:mdsp_memset, lib), Cint, (Ptr{Cvoid}, Cint, Csize_t, Ptr{Cvoid}), a.ptr, byte, length(a) * sizeof(eltype(a)), C_NULL)); a
end

function upload(x::Array{T,N}) where {T,N}
    d = DeviceArray{T}(size(x))
    GC.@preserve x check(ccall((:mdsp_memcpy_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), d.ptr, pointer(x), sizeof(x), C_NULL))
    d
end
function download(d::DeviceArray{T,N}) where {T,N}
    x = Array{T,N}(undef, d.dims)
    GC.@preserve x check(ccall((:mdsp_memcpy_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), pointer(x), d.ptr, sizeof(x), C_NULL))
    x
end
todevice(x::DeviceArray, ::Type{T}) where {T} = eltype(x) == T ? x : upload(convert(Array{T}, download(x)))
todevice(x::AbstractArray, ::Type{T}) where {T} = upload(convert(Array{T}, x))
back(y::DeviceArray, like::DeviceArray) = y
back(y::DeviceArray, like) = download(y)
ncolumns(x) = length(x) ÷ max(size(x, 1), 1)

# page-locked host memory: hipHostMalloc'ed arrays, or an existing Array page-locked in place (hipHostRegister)
function pinned_array(::Type{T}, dims::Int...) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_host_alloc, lib), Cint, (Ref{Ptr{Cvoid}}, Csize_t), p, prod(dims) * sizeof(T)))
    a = unsafe_wrap(Array, Ptr{T}(p[]), dims)
    finalizer(x -> ccall((:mdsp_host_free, lib), Cint, (Ptr{Cvoid},), pointer(x)), a)
    a
end
pin!(x::Array) = (check(ccall((:mdsp_host_register, lib), Cint, (Ptr{Cvoid}, Csize_t), pointer(x), sizeof(x))); x)
unpin!(x::Array) = (check(ccall((:mdsp_host_unregister, lib), Cint, (Ptr{Cvoid},), pointer(x))); x)

# ---------------------------------------------------------------------------------------------- index arithmetic
nextfastfft(n::Integer) = Int(ccall((:mdsp_nextfastfft, lib), Int64, (Int64,), n))                       # util.jl:134
optimalfftfiltlength(nb, nx) = Int(ccall((:mdsp_optimal_fft_len, lib), Int64, (Int64, Int64), nb, nx))  # dspbase.jl:268
framecount(len, n, noverlap) = Int(ccall((:mdsp_frame_count, lib), Int64, (Int64, Int64, Int64), len, n, noverlap))
outputlength(inlen::Integer, ratio::Union{Integer,Rational}, ϕ::Integer) =                                 # stream_filt.jl:317
    Int(ccall((:mdsp_outputlength, lib), Int64, (Int64, Int64, Int64, Int64), inlen, numerator(ratio), denominator(ratio), ϕ))
inputlength(outlen::Integer, ratio::Union{Integer,Rational}, ϕ::Integer, r::RoundingMode=RoundDown) =      # stream_filt.jl:358
    Int(ccall((:mdsp_inputlength, lib), Int64, (Int64, Int64, Int64, Int64, Cint), outlen, numerator(ratio), denominator(ratio), ϕ,
              (r == RoundUp || r == RoundFromZero) ? 1 : 0))
# block geometry of _fftfilt! (Filters/filt.jl:490, :504-517) for block `iblock` (0-based): what the parity tests compare bit for bit
function ols_block_geometry(nb, nfft, nx, iblock)
    o = ntuple(_ -> Ref{Int64}(0), 5)
    check(ccall((:mdsp_ols_block_geometry, lib), Cint, (Int64, Int64, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                nb, nfft, nx, iblock, o[1], o[2], o[3], o[4], o[5]))
    (off = Int(o[1][]), npadbefore = Int(o[2][]), xstart = Int(o[3][]), n = Int(o[4][]), nout = Int(o[5][]))
end

const SMALL_FILT_CUTOFF = 66   # dspbase.jl:3

# ---------------------------------------------------------------------------------------------- overlap-save filt / conv
mutable struct OlsPlan
    h::Ptr{Cvoid}
    function OlsPlan(taps::Vector{T}, nfft::Integer, nx::Integer, mode::Integer, engine=ENGINE_AUTO) where {T}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve taps check(ccall((:mdsp_ols_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Cint),
                                      p, pointer(taps), length(taps), nfft, nx, mdtype(T), mode, engine))
        o = new(p[])
        finalizer(x -> ccall((:mdsp_ols_plan_destroy, lib), Cint, (Ptr{Cvoid},), x.h), o)
        o
    end
end
# (nfft, block length L, engine) as the reference would use them / as the fused engine actually executes a long filter
function plan_info(h::Ptr{Cvoid})
    nfft, L, e = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    check(ccall((:mdsp_ols_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}), h, nfft, L, e))
    (nfft = Int(nfft[]), L = Int(L[]), engine = Int(e[]))
end
function plan_geometry(h::Ptr{Cvoid})
    nfft, L, parts = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    check(ccall((:mdsp_ols_plan_geometry, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}), h, nfft, L, parts))
    (nfft = Int(nfft[]), L = Int(L[]), partitions = Int(parts[]))
end
# the same without a plan or a device: what a plan for these arguments would execute (rows > 0: the rows form of the multi-pass engine)
function ols_geometry_for(nb::Integer, nfft::Integer, nx::Integer, ::Type{T}, mode::Integer=OLS_FILT, engine::Integer=ENGINE_AUTO) where {T}
    en, L, parts, eng, rows = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:mdsp_ols_geometry_for, lib), Cint, (Int64, Int64, Int64, Cint, Cint, Cint, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cint}, Ref{Cint}),
                nb, nfft, nx, mdtype(T), mode, engine, en, L, parts, eng, rows))
    (nfft = Int(en[]), L = Int(L[]), partitions = Int(parts[]), engine = Int(eng[]), rows = Int(rows[]))
end
# the windows the whole-column and host calls run: (tile, lead) == (L, nb - 1) except on tiled plans (real Float32, nfft 2048, 249 .. 257 taps: (1792, 256))
function plan_tile(h::Ptr{Cvoid})
    tile, lead = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_ols_plan_tile, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), h, tile, lead))
    (tile = Int(tile[]), lead = Int(lead[]))
end
function ols_tile_for(nb::Integer, nfft::Integer, nx::Integer, ::Type{T}, mode::Integer=OLS_FILT, engine::Integer=ENGINE_AUTO) where {T}
    tile, lead = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_ols_tile_for, lib), Cint, (Int64, Int64, Int64, Cint, Cint, Cint, Ref{Int64}, Ref{Int64}),
                nb, nfft, nx, mdtype(T), mode, engine, tile, lead))
    (tile = Int(tile[]), lead = Int(lead[]))
end
# whether a launch of a tiled plan over `columns` columns of nx samples / nout outputs runs the streaming cache policy (the footprint rule, knob MDSP_OLS_STREAM)
function ols_stream_for(nx::Integer, nout::Integer, columns::Integer, ::Type{T}) where {T}
    streaming = Ref{Cint}(0)
    check(ccall((:mdsp_ols_stream_for, lib), Cint, (Int64, Int64, Int64, Cint, Ref{Cint}), nx, nout, columns, mdtype(T), streaming))
    streaming[] != 0
end
# the run schedule of a fused overlap-save launch of `units` units on `slots` slots (short runs for the streaming tiled launch, else one run per slot)
function ols_run_for(units::Integer, slots::Integer, streaming_tiled::Bool)
    run_len, niter = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_ols_run_for, lib), Cint, (Int64, Int64, Cint, Ref{Int64}, Ref{Int64}), units, slots, streaming_tiled ? 1 : 0, run_len, niter))
    (run_len = Int(run_len[]), niter = Int(niter[]))
end

# The function-style entry points build a plan per call in the reference (cheap FFTW plans); here the plan comes from the LIBRARY's LRU
# (mdsp_ols_plan_cached: keyed by device, thread, stream and the contents of the taps) -- ~45 us per call instead of ~1 ms.  The handle is
# borrowed: no finalizer, never destroyed from here.
function cached_ols_plan(taps::Vector{T}, nfft::Integer, nx::Integer, mode::Integer, engine=ENGINE_AUTO) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve taps check(ccall((:mdsp_ols_plan_cached, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Cint, Ptr{Cvoid}),
                                  p, pointer(taps), length(taps), nfft, nx, mdtype(T), mode, engine, C_NULL))
    p[]
end

function ols_exec!(y::DeviceArray, plan::Ptr{Cvoid}, x::DeviceArray, nout::Integer)
    nx = size(x, 1)
    check(ccall((:mdsp_ols_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                plan, x.ptr, nx, ncolumns(x), nx, y.ptr, nout, nout, C_NULL))
    y
end
function ols_exec_host!(y::Array, plan::Ptr{Cvoid}, x::Array, nout::Integer; pinned::Bool=false)
    nx = size(x, 1)
    GC.@preserve x y check(ccall((:mdsp_ols_exec_host, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Cint),
                                 plan, pointer(x), nx, ncolumns(x), nx, pointer(y), nout, nout, pinned ? HOST_PINNED : Cint(0)))
    y
end
# blocks [first, first + count) of the same block grid from a slice of the signal (time-axis split over GPUs; no collective)
function ols_exec_range!(ys::DeviceArray, plan::Ptr{Cvoid}, xs::DeviceArray, xs_first::Integer, nx::Integer, first::Integer, count::Integer, nout::Integer)
    check(ccall((:mdsp_ols_exec_range, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}),
                plan, xs.ptr, xs_first, length(xs), nx, ys.ptr, first, count, nout, C_NULL))
    ys
end
# the exact contents of `tmp1` before the forward transform (filt.jl:509-510) for blocks [first, first + count): parity tests
function ols_segment(plan::Ptr{Cvoid}, x::DeviceArray{T}, first::Integer, count::Integer) where {T}
    out = DeviceArray{T}((plan_info(plan).nfft, Int(count)))
    check(ccall((:mdsp_ols_segment, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                plan, x.ptr, size(x, 1), first, count, out.ptr, C_NULL))
    out
end

# fftfilt(b, x[, nfft]) / fftfilt!(out, b, x[, nfft])   Filters/filt.jl:458-476, _fftfilt! :479-521
# Device arrays: one launch sequence on resident data.  Host Arrays: the chunked H2D || kernel || D2H pipeline (same block grid, so
# both return bit-identical results).
# (filters of any length: beyond the partitioned kernels -- 16384 Float32 / 8192 Float64 taps -- the plan runs blocks of 2^20 points on the multi-pass engine)
function fftfilt(b::AbstractVector{H}, x::DeviceArray{T}, nfft::Integer=optimalfftfiltlength(length(b), length(x))) where {H<:Real,T<:Real}
    W = fftintype(promote_type(H, T))
    xd = todevice(x, W)
    nx = size(xd, 1)
    plan = cached_ols_plan(convert(Vector{W}, b), nfft, nx, OLS_FILT)
    ols_exec!(DeviceArray{W}(size(xd)), plan, xd, nx)
end
function fftfilt(b::AbstractVector{H}, x::AbstractArray{T}, nfft::Integer=optimalfftfiltlength(length(b), length(x));
                 pinned::Bool=false) where {H<:Real,T<:Real}
    W = fftintype(promote_type(H, T))
    xh = convert(Array{W}, x)                                  # column-major (n, cols...): exactly the layout the C ABI takes
    plan = cached_ols_plan(convert(Vector{W}, b), nfft, size(xh, 1), OLS_FILT)
    ols_exec_host!(similar(xh), plan, xh, size(xh, 1); pinned)
end
function fftfilt!(out::AbstractArray, b::AbstractVector{<:Real}, x::AbstractArray{<:Real}, nfft::Integer=optimalfftfiltlength(length(b), length(x)))
    size(out) == size(x) || throw(ArgumentError("out and x must be the same size"))            # filt.jl:474
    copyto!(out, fftfilt(b, x, nfft))
end

# filt(b, a::Number, x) / filt!(out, b, a, x) / tdfilt(h, x) / tdfilt!(out, h, x)   dspbase.jl:14-66, filt.jl:431-443 (FIR only on the device)
function filt(b::AbstractVector, a::Number, x::Union{AbstractArray{T},DeviceArray{T}}) where {T}
    isempty(b) && throw(ArgumentError("filter vector b must be non-empty"))
    a == 0 && throw(ArgumentError("filter vector a[1] must be nonzero"))
    W = fftintype(promote_type(eltype(b), typeof(a), T))
    if promote_type(eltype(b), typeof(a)) <: Complex       # complex taps (plain product, no conjugate): explicit tap dtype, the signal keeps its class
        Tx = T <: Complex ? W : real(W)
        ctaps = convert(Vector{W}, a == 1 ? b : b ./ a)
        xc = todevice(x, Tx)
        yc = DeviceArray{W}(size(xc))
        n = size(xc, 1)
        GC.@preserve ctaps check(ccall((:mdsp_tdfir_exec_t, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                                       pointer(ctaps), length(ctaps), mdtype(W), mdtype(Tx), xc.ptr, n, ncolumns(xc), n, yc.ptr, n, C_NULL))
        return back(yc, x)
    end
    taps = convert(Vector{real(W)}, a == 1 ? b : b ./ a)
    xd = todevice(x, W)
    y = DeviceArray{W}(size(xd))
    nx = size(xd, 1)
    GC.@preserve taps check(ccall((:mdsp_tdfir_exec, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                                  pointer(taps), length(taps), mdtype(W), xd.ptr, nx, ncolumns(xd), nx, y.ptr, nx, C_NULL))
    back(y, x)
end
filt(b::AbstractVector, a::AbstractVector, x) = length(a) == 1 ? filt(b, a[1], x) :
    throw(UnsupportedError("IIR filt(b, a, x) is a serial recursion; only FIR (scalar a) runs on the device"))
function filt!(out::AbstractArray, b::AbstractVector, a::Union{Number,AbstractVector}, x::AbstractArray)
    size(out) == size(x) || throw(ArgumentError("output size $(size(out)) must match input size $(size(x))"))   # dspbase.jl:32
    copyto!(out, filt(b, a, x))
end
tdfilt(h::AbstractVector{H}, x) where {H} = filt(h, one(H), x)                      # filt.jl:431
function tdfilt!(out::AbstractArray, h::AbstractVector, x::AbstractArray)
    size(out) == size(x) || throw(ArgumentError("out must be the same size as x"))
    copyto!(out, tdfilt(h, x))
end

# filt(b, x) / filt!(out, b, x): FFT path for real taps longer than SMALL_FILT_CUTOFF, time domain otherwise   filt.jl:445-446, :525-555
function filt(b::AbstractVector{<:Real}, x::Union{AbstractArray{<:Real},DeviceArray{<:Real}})
    length(b) > SMALL_FILT_CUTOFF ? fftfilt(b, x, optimalfftfiltlength(length(b), size(x, 1))) : tdfilt(b, x)
end
function filt!(out::AbstractArray, b::AbstractVector{<:Real}, x::AbstractArray{<:Real})
    size(out) == size(x) || throw(ArgumentError("out must be the same size as x"))             # filt.jl:531
    copyto!(out, filt(b, x))
end

# conv(u, v; algorithm) / conv!(out, u, v; algorithm)   dspbase.jl:709-792 (vectors; :direct for small / integer inputs goes to the N-d entry)
function conv(u::AbstractVector{Tu}, v::AbstractVector{Tv}; algorithm=:auto) where {Tu<:Number,Tv<:Number}
    T = promote_type(Tu, Tv)
    W = fftintype(T)
    nu, nv = length(u), length(v)
    (nu == 0 || nv == 0) && return zeros(T, max(nu + nv - 1, 0))
    alg = algorithm
    alg === :auto && (alg = T <: Union{Float32,Float64,ComplexF32,ComplexF64} ? :fast : :direct)
    alg === :fast && (alg = nu * nv < 2^16 ? :direct : :fft)
    alg === :direct && return convnd(reshape(u, :, 1), reshape(v, :, 1), :direct)[:, 1]
    big, small = nu >= nv ? (u, v) : (v, u)
    os = optimalfftfiltlength(length(small), length(big))
    alg === :fft && (alg = os < nu + nv - 1 ? :fft_overlapsave : :fft_simple)
    alg in (:fft_overlapsave, :fft_simple) ||
        throw(ArgumentError("algorithm must be :auto, :fast, :direct, :fft, :fft_simple, or :fft_overlapsave"))
    nfft = alg === :fft_simple ? nextfastfft(nu + nv - 1) : os
    plan = cached_ols_plan(convert(Vector{W}, small), nfft, length(big), OLS_CONV)
    download(ols_exec!(DeviceArray{W}((nu + nv - 1,)), plan, todevice(big, W), nu + nv - 1))
end

# conv(u, v; algorithm) for arrays   dspbase.jl:709-792: _conv_kern_fft! (:611-644) / _conv_td! (:646-660) on the device.
# Julia arrays are column-major, which is the layout the C ABI takes: sizes are passed as they are.
function convnd(u::AbstractArray{Tu,N}, v::AbstractArray{Tv,N}, alg::Symbol) where {Tu<:Number,Tv<:Number,N}
    T = promote_type(Tu, Tv)
    W = T <: Union{Float32,Float64,ComplexF32,ComplexF64} ? T : (T <: Complex ? ComplexF64 : Float64)
    so = size(u) .+ size(v) .- 1
    ud, vd, out = todevice(u, W), todevice(v, W), DeviceArray{W}(so)
    su, sv = collect(Int64, size(u)), collect(Int64, size(v))
    if alg === :direct
        GC.@preserve su sv check(ccall((:mdsp_convnd_direct, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                                       ud.ptr, pointer(su), vd.ptr, pointer(sv), N, mdtype(W), out.ptr, C_NULL))
    else
        GC.@preserve su sv check(ccall((:mdsp_convnd_fft, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                                       ud.ptr, pointer(su), vd.ptr, pointer(sv), N, mdtype(W), out.ptr, C_NULL))
    end
    res = download(out)
    T === W ? res : round.(T, res)                     # integer eltypes: exact in Float64 below 2^53
end
function conv(u::AbstractArray{Tu,N}, v::AbstractArray{Tv,N}; algorithm=:auto) where {Tu<:Number,Tv<:Number,N}
    T = promote_type(Tu, Tv)
    (isempty(u) || isempty(v)) && return zeros(T, max.(size(u) .+ size(v) .- 1, 0))
    alg = algorithm
    alg === :auto && (alg = T <: Union{Float32,Float64,ComplexF32,ComplexF64} ? :fast : :direct)
    alg === :fast && (alg = length(u) * length(v) < 2^16 ? :direct : :fft)
    alg in (:direct, :fft, :fft_simple, :fft_overlapsave) ||
        throw(ArgumentError("algorithm must be :auto, :fast, :direct, :fft, :fft_simple, or :fft_overlapsave"))
    convnd(u, v, alg === :direct ? :direct : :fft)
end
# rank promotion with trailing singleton dimensions   dspbase.jl:784-792
function conv(A::AbstractArray{<:Number,M}, B::AbstractArray{<:Number,N}; kwargs...) where {M,N}
    M < N ? conv(reshape(A, size(A)..., ntuple(_ -> 1, N - M)...), B; kwargs...) :
            conv(A, reshape(B, size(B)..., ntuple(_ -> 1, M - N)...); kwargs...)
end
# separable 2-d kernel   dspbase.jl:801-818
conv(u::AbstractVector, v::AbstractMatrix{<:Number}, A::AbstractMatrix) = size(v, 1) == 1 ? conv(reshape(u, :, 1) * v, A) :
    throw(ArgumentError("conv(u, v', A): v must be a row vector"))
function conv!(out::AbstractArray, u::AbstractArray, v::AbstractArray; algorithm=:auto)          # dspbase.jl:709-750
    res = conv(u, v; algorithm)
    size(out) == size(res) || throw(ArgumentError("output size $(size(out)) must equal input sizes minus one: $(size(res))"))   # :754
    copyto!(out, res)
end

# xcorr(u, v; padmode, scaling)   dspbase.jl:867-898
function xcorr(u::AbstractVector, v::AbstractVector=u; padmode::Symbol=:none, scaling::Symbol=:none)
    su, sv = length(u), length(v)
    scaling === :biased && su != sv && throw(DimensionMismatch("scaling only valid for vectors of same length"))
    padmode in (:none, :longest) || throw(ArgumentError("padmode keyword argument must be either :none or :longest"))
    if padmode === :longest
        n = max(su, sv)
        u, v = vcat(u, zeros(eltype(u), n - su)), vcat(v, zeros(eltype(v), n - sv))
    end
    res = conv(u, conj.(reverse(v)))
    scaling === :biased ? res ./ su : res
end

# hilbert(x)   util.jl:31-87: analytic signal of every real column
function hilbert(x::Union{AbstractVecOrMat{T},DeviceArray{T}}) where {T<:Real}
    S = fftintype(T)
    xd = todevice(x, S)
    n = size(xd, 1)
    out = DeviceArray{fftouttype(S)}(size(xd))
    n > 0 && check(ccall((:mdsp_hilbert, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                         xd.ptr, n, ncolumns(xd), n, mdtype(S), out.ptr, n, C_NULL))
    back(out, x)
end

# unwrap / unwrap!   unwrap.jl:17-34, the dims::Integer form: accumulate!(unwrap_kernel(range), y, m; dims) as an integer prefix sum on the device.
# A Julia array unwrapped along d is (inner, len, outer) = (prod(size[1:d-1]), size[d], prod(size[d+1:end])) as it lies in memory: no transposes.
function unwrap_geometry(inner::Integer, len::Integer, outer::Integer, ::Type{T}; segments::Integer=0) where {T<:Union{Float32,Float64}}
    route, S, seglen, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_unwrap_geometry_for, lib), Cint, (Int64, Int64, Int64, Cint, Int64, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                inner, len, outer, mdtype(T), segments, route, S, seglen, ws))
    (route=Int(route[]), segments=Int(S[]), seglen=Int(seglen[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code (same geometry, same operator): what the CPU tests compare with the serial recurrence
function unwrap_emulate(m::Array{T,N}, d::Integer; range=2T(pi), segments::Integer=0) where {T<:Union{Float32,Float64},N}
    y = similar(m)
    GC.@preserve y m check(ccall((:mdsp_unwrap_emulate_host, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cdouble, Int64),
                                 pointer(m), pointer(y), prod(size(m)[1:d-1]), size(m, d), prod(size(m)[d+1:end]), mdtype(T), Float64(T(range)), segments))
    y
end
function unwrap!(y::DeviceArray{T,N}, m::DeviceArray{T,N}; dims=nothing, range=2T(pi), segments::Integer=0, kwargs...) where {T,N}
    if dims === nothing
        N != 1 && throw(ArgumentError("`unwrap!`: required keyword parameter dims missing"))
        dims = 1
    end
    if !(dims isa Integer)
        dims == 1:N && throw(UnsupportedError("unwrap over all dimensions (dims = 1:N, unwrap_nd!) is not accelerated: use DSP.jl's CPU path"))
        throw(ArgumentError("`unwrap!`: Invalid dims specified: $dims"))
    end
    T <: Union{Float32,Float64} || throw(MethodError(unwrap!, (y, m)))
    size(y) == size(m) || throw(ArgumentError("unwrap!: y and m must have the same size"))
    1 <= dims <= N || throw(ArgumentError("`unwrap!`: Invalid dims specified: $dims"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_unwrap_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Cint, Cdouble, Int64),
                h, prod(size(m)[1:dims-1]), size(m, dims), prod(size(m)[dims+1:end]), mdtype(T), Float64(T(range)), segments))
    try
        route, S, seglen, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_unwrap_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], route, S, seglen, ws))
        check(ccall((:mdsp_unwrap_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], m.ptr, y.ptr, C_NULL))
    finally
        ccall((:mdsp_unwrap_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    y
end
unwrap!(m::DeviceArray; kwargs...) = unwrap!(m, m; kwargs...)
unwrap(m::DeviceArray{T,N}; kwargs...) where {T,N} = unwrap!(DeviceArray{T}(size(m)), m; kwargs...)
unwrap(m::AbstractArray{T}; kwargs...) where {T<:Union{Float32,Float64}} = download(unwrap!(upload(Array(m)); kwargs...))
function unwrap!(y::AbstractArray{T,N}, m::AbstractArray{T,N}; kwargs...) where {T<:Union{Float32,Float64},N}
    copyto!(y, unwrap(m; kwargs...))
end
unwrap!(m::AbstractArray{T}; kwargs...) where {T<:Union{Float32,Float64}} = unwrap!(m, m; kwargs...)

# Biquad / SecondOrderSections   Filters/filt.jl:35-96, :188-210, :341-360: the cascade of second-order sections on the device (mdsp_sos_*).
# coef is 5 x K (b0 b1 b2 a1 a2 down each column, a0 = 1: the K x 5 rows the C ABI takes, as they lie in memory), gain === nothing for a Biquad.
# From DSP.jl's types: coef = [getfield(q, f) for f in (:b0, :b1, :b2, :a1, :a2), q in f.biquads], gain = f.g.  T is the working type
# promote_type(T, G, S); a complex signal runs as two real lines per column.
const SosTypes = Union{Float32,Float64,ComplexF32,ComplexF64}
function sos_geometry(K::Integer, ::Type{T}, n::Integer, ncols::Integer; segments::Integer=0) where {T<:SosTypes}
    S, seglen, tile, run, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_sos_geometry_for, lib), Cint, (Int64, Cint, Int64, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                K, mdtype(T), n, ncols, segments, S, seglen, tile, run, ws))
    (segments=Int(S[]), seglen=Int(seglen[]), tile=Int(tile[]), run=Int(run[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code (same cut, tiles, scan order and arithmetic): equal to the device bit for bit.  state: (2, K, ncols) or nothing
function sos_emulate(coef::Matrix{Float64}, gain::Union{Nothing,Real}, x::Array{T}; state::Union{Nothing,Array{T}}=nothing, reverse::Bool=false,
                     segments::Integer=0) where {T<:SosTypes}
    size(coef, 1) == 5 || throw(ArgumentError("coef must be 5 x K"))
    y = similar(x)
    n, ncols = size(x, 1), div(length(x), max(size(x, 1), 1))
    GC.@preserve x y state coef check(ccall((:mdsp_sos_emulate_host, lib), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cdouble}, Int64, Cdouble, Cint, Cint, Int64, Int64, Int64, Cint),
        pointer(x), n, pointer(y), n, state === nothing ? C_NULL : pointer(state), pointer(coef), size(coef, 2), gain === nothing ? 1.0 : Float64(gain),
        gain === nothing ? 0 : 1, mdtype(T), n, ncols, segments, reverse ? 1 : 0))
    y
end
# filt!(y, f, x) on device columns; y === x filters in place.  state: a (2, K, ncols) DeviceArray{T}, read as the state in front of the first sample and
# overwritten with the state behind the last (the DF2TFilter forms), or nothing (zero state, end state dropped).  reverse: the backward pass of filtfilt.
function sosfilt!(y::DeviceArray{T}, coef::Matrix{Float64}, gain::Union{Nothing,Real}, x::DeviceArray{T}; state::Union{Nothing,DeviceArray{T}}=nothing,
                  reverse::Bool=false, segments::Integer=0) where {T<:SosTypes}
    size(coef, 1) == 5 || throw(ArgumentError("coef must be 5 x K"))
    size(x) == size(y) || throw(DimensionMismatch("out size must match x"))                                    # filt.jl:54
    K, n, ncols = size(coef, 2), size(x, 1), ncolumns(x)
    state === nothing || size(state)[1:2] == (2, K) && div(length(state), 2K) == ncols || throw(ArgumentError("state size must match x"))   # :190
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve coef check(ccall((:mdsp_sos_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cdouble}, Int64, Cdouble, Cint, Cint, Int64, Int64, Int64),
                                  h, pointer(coef), K, gain === nothing ? 1.0 : Float64(gain), gain === nothing ? 0 : 1, mdtype(T), n, ncols, segments))
    try
        S, seglen, tile, run, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_sos_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], S, seglen, tile, run, ws))
        check(ccall((:mdsp_sos_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                    h[], x.ptr, n, y.ptr, n, state === nothing ? C_NULL : state.ptr, reverse ? 1 : 0, C_NULL))
    finally
        ccall((:mdsp_sos_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    y
end
sosfilt(coef::Matrix{Float64}, gain, x::DeviceArray{T}; kwargs...) where {T<:SosTypes} = sosfilt!(DeviceArray{T}(size(x)), coef, gain, x; kwargs...)
sosfilt(coef::Matrix{Float64}, gain, x::AbstractArray{T}; kwargs...) where {T<:SosTypes} = download(sosfilt!(upload(Array(x)), coef, gain, upload(Array(x)); kwargs...))

# freqresp / phaseresp / grpdelay   Filters/response.jl:27-52, :73-76, :96-111: a rational function at nw points of the unit circle (mdsp_resp_*).
# form RESP_POLY: num = b, den = a in powers of z^-1 (den === nothing: FIR), y = exp(-iw) with RESP_NEG; RESP_SECTIONS: num = the 5 x K table of
# sosfilt, gain = f.g; RESP_ZPK: num / den = zeros / poles as (re, im) pairs (reinterpret(Float64, z)), gain = f.k.  T is the REAL type of the working
# type: Float32 when coefficients and w are, Float64 otherwise.  From DSP.jl's types:
#   freqresp(f::PolynomialRatio, w) = resp(RESP_POLY, coefb(f), coefa(f), w; flags=RESP_NEG)
#   phaseresp                        = unwrap!(resp(...; out_mode=RESP_ANGLE))
#   grpdelay: c = xcorr(b, a);         resp(RESP_POLY, c, c, w; flags=RESP_NEG | RESP_DERIV, out_mode=RESP_REAL_MINUS, cminus=length(a) - 1)
const RESP_POLY, RESP_SECTIONS, RESP_ZPK = Cint(0), Cint(1), Cint(2)
const RESP_DERIV, RESP_NEG = Cint(1), Cint(2)
const RESP_COMPLEX, RESP_ANGLE, RESP_REAL_MINUS = Cint(0), Cint(1), Cint(2)
const RESP_W, RESP_POINTS = Cint(0), Cint(1)
const RespTypes = Union{Float32,Float64}
resp_count(form, v) = v === nothing ? 0 : form == RESP_POLY ? length(v) : form == RESP_SECTIONS ? div(length(v), 5) : div(length(v), 2)
function resp_geometry(form::Integer, ::Type{T}, ncoef::Integer, has_den::Bool, nw::Integer; chunks::Integer=0) where {T<:RespTypes}
    C, L, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_resp_geometry_for, lib), Cint, (Cint, Cint, Int64, Cint, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                form, mdtype(T), ncoef, has_den ? 1 : 0, nw, chunks, C, L, ws))
    (chunks=Int(C[]), chunk_len=Int(L[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code (same cut, chunk order, squaring chain and operators) at given points: equal to the device bit for bit
function resp_emulate(form::Integer, num::Array{Float64}, den::Union{Nothing,Array{Float64}}, points::Array{Complex{T}}; gain::Real=1.0, flags::Integer=0,
                      out_mode::Integer=RESP_COMPLEX, cminus::Real=0.0, chunks::Integer=0) where {T<:RespTypes}
    out = out_mode == RESP_COMPLEX ? similar(points) : Array{T}(undef, size(points))
    GC.@preserve num den points out check(ccall((:mdsp_resp_emulate_host, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Int64, Int64),
        pointer(points), pointer(out), form, flags, out_mode, mdtype(T), pointer(num), resp_count(form, num), den === nothing ? C_NULL : pointer(den),
        resp_count(form, den), Float64(gain), Float64(cminus), length(points), chunks))
    out
end
# one plan over the device array of frequencies (in_mode = RESP_W, real) or of points (RESP_POINTS, complex); the result has the shape of `arg`
function resp(form::Integer, num::Array{Float64}, den::Union{Nothing,Array{Float64}}, arg::DeviceArray{A}; gain::Real=1.0, flags::Integer=0,
              out_mode::Integer=RESP_COMPLEX, cminus::Real=0.0, chunks::Integer=0) where {A<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    T = real(A)
    in_mode = A <: Complex ? RESP_POINTS : RESP_W
    out = out_mode == RESP_COMPLEX ? DeviceArray{Complex{T}}(size(arg)) : DeviceArray{T}(size(arg))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve num den check(ccall((:mdsp_resp_plan_create, lib), Cint,
        (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Int64, Int64),
        h, form, flags, out_mode, in_mode, mdtype(T), pointer(num), resp_count(form, num), den === nothing ? C_NULL : pointer(den),
        resp_count(form, den), Float64(gain), Float64(cminus), length(arg), chunks))
    try
        C, L, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_resp_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], C, L, ws))
        check(ccall((:mdsp_resp_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], arg.ptr, out.ptr, C_NULL))
    finally
        ccall((:mdsp_resp_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    out
end
resp(form::Integer, num, den, w::AbstractArray{<:Real}; kwargs...) = download(resp(form, Float64.(num), den === nothing ? nothing : Float64.(den), upload(Array(float.(w))); kwargs...))
# impresp / stepresp (response.jl:127-140) on a section table: filt of a Float64 impulse or step
impresp(coef::Matrix{Float64}, gain, n::Integer=100) = sosfilt(coef, gain, setindex!(zeros(n), 1, 1))
stepresp(coef::Matrix{Float64}, gain, n::Integer=100) = sosfilt(coef, gain, ones(n))

# ---------------------------------------------------------------------------------------------- util.jl:138-220, :316-430
# COMMON DSP TOOLS and DELAY FINDING UTILITIES: deterministic device reductions (mdsp_reduce_*: store, then sum; Float64 additions in a fixed order)
# and a zero-filling shift that is correct in place (mdsp_shift_*).
db2pow(a::Real) = exp10(a / 10)          # :154
db2amp(a::Real) = exp10(a / 20)          # :162
pow2db(a::Real) = 10 * log10(a)          # :170
amp2db(a::Real) = 20 * log10(a)          # :178

const REDUCE_SUMABS2, REDUCE_SUMABS2_W, REDUCE_ABSARGMAX = Cint(0), Cint(1), Cint(2)
const SHIFT_AUTO, SHIFT_DISJOINT, SHIFT_HALO, SHIFT_STAGED = Cint(0), Cint(1), Cint(2), Cint(3)

function reduce_geometry(inner::Integer, len::Integer, outer::Integer, op::Integer, ::Type{T}; segments::Integer=0) where {T}
    route, S, seglen, depth, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_reduce_geometry_for, lib), Cint, (Int64, Int64, Int64, Cint, Cint, Int64, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                inner, len, outer, op, mdtype(T), segments, route, S, seglen, depth, ws))
    (route=Int(route[]), segments=Int(S[]), seglen=Int(seglen[]), depth=Int(depth[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code (same geometry, operators and order of additions): R = Float64 for the sums, Int64 for ABSARGMAX
function reduce_emulate(x::Array{T}, inner::Integer, len::Integer, outer::Integer, op::Integer; step::Real=0.0, centre::Integer=0, segments::Integer=0,
                        phase::Integer=0) where {T}
    words = op == REDUCE_SUMABS2 ? 1 : 2
    out = op == REDUCE_ABSARGMAX ? zeros(Int64, words, inner * outer) : zeros(Float64, words, inner * outer)
    reached = Ref{Int64}(0)
    GC.@preserve x out check(ccall((:mdsp_reduce_emulate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Cdouble, Int64, Int64, Int64, Ref{Int64}),
                                   pointer(x), pointer(out), inner, len, outer, op, mdtype(T), Float64(step), centre, segments, phase, reached))
    out, Int(reached[])
end
# one plan, one exec: `out` holds 1 (SUMABS2) or 2 eight-byte words per line
function reduce_exec!(out::DeviceArray, x::DeviceArray{T}, inner::Integer, len::Integer, outer::Integer, op::Integer; step::Real=0.0, centre::Integer=0,
                      segments::Integer=0) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_reduce_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Cint, Cint, Cdouble, Int64, Int64),
                h, inner, len, outer, op, mdtype(T), Float64(step), centre, segments))
    try
        route, S, seglen, depth, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_reduce_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], route, S, seglen, depth, ws))
        check(ccall((:mdsp_reduce_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], x.ptr, out.ptr, C_NULL))
    finally
        ccall((:mdsp_reduce_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    out
end
const ReduceTypes = Union{Float32,Float64,ComplexF32,ComplexF64}
_sumabs2(x::DeviceArray{T}, inner, len, outer) where {T<:ReduceTypes} = download(reduce_exec!(DeviceArray{Float64}((inner * outer,)), x, inner, len, outer, REDUCE_SUMABS2))

# rms(s; dims)   :186-192 (dims = : or one dimension)
function rms(s::DeviceArray{T,N}; dims=:) where {T<:ReduceTypes,N}
    R = real(T)
    if dims === (:)
        length(s) == 0 && return R(NaN)
        return R(sqrt(_sumabs2(s, 1, length(s), 1)[1] / length(s)))
    end
    dims isa Integer || throw(UnsupportedError("rms over several dimensions is not accelerated: use DSP.jl's CPU path"))
    1 <= dims <= N || throw(ArgumentError("rms: Invalid dims specified: $dims"))
    inner, len, outer = prod(size(s)[1:dims-1]), size(s, dims), prod(size(s)[dims+1:end])
    osz = ntuple(k -> k == dims ? 1 : size(s, k), N)
    (inner * outer == 0 || len == 0) && return fill(R(NaN), osz)
    reshape(R.(sqrt.(_sumabs2(s, inner, len, outer) ./ len)), osz)
end
rms(s::AbstractArray{T}; kwargs...) where {T<:ReduceTypes} = rms(upload(Array(s)); kwargs...)
rms(s::AbstractArray{T}; kwargs...) where {T<:Union{Integer,Complex{<:Integer}}} = rms(float.(s); kwargs...)
# rmsfft(f)   :200
rmsfft(f::DeviceArray{T}) where {T<:Complex} = length(f) == 0 ? real(T)(NaN) : real(T)(sqrt(_sumabs2(f, 1, length(f), 1)[1]) / length(f))
rmsfft(f::AbstractArray{T}) where {T<:Complex} = rmsfft(upload(convert(Array{fftouttype(T)}, f)))

# meanfreq(x, fs)   :211-220: one pass over the bins of rfft(x) forms sum(pxx .* freqrg) and sum(pxx); no |X|^2 array is written
function meanfreq(x::AbstractVector{T}, fs=2π) where {T<:Real}
    len = length(x)
    len > 0 || throw(ArgumentError("meanfreq: empty signal"))
    X = stft(x, len, 0; nfft=len, window=nothing, onesided=true)
    bins = X isa DeviceArray ? X : upload(vec(Array(X)))
    R = promote_type(real(eltype(bins)), typeof(fs / len))
    sums = download(reduce_exec!(DeviceArray{Float64}((2,)), bins, 1, length(bins), 1, REDUCE_SUMABS2_W; step=Float64(fs / len)))
    R(sums[1] / sums[2])
end

# finddelay(x, y)   :336-347: xcorr(y, x), then one device arg-max with the reference's tie rules (nearest to length(x), then the smaller index)
function finddelay(x::AbstractVector{<:Real}, y::AbstractVector{<:Real})
    (isempty(x) || isempty(y)) && throw(ArgumentError("reducing over an empty collection is not allowed"))
    s = xcorr(y, x)
    sd = s isa DeviceArray ? s : upload(convert(Array{fftintype(eltype(s))}, s))
    centre = length(x) - 1                                     # center_idx = length(x), 0-based
    rec = download(reduce_exec!(DeviceArray{Int64}((2,)), sd, 1, length(sd), 1, REDUCE_ABSARGMAX; centre=centre))
    (rec[2] != 0 || rec[1] < 0) && throw(ArgumentError("finddelay: the cross-correlation holds NaN"))
    centre - Int(rec[1])
end

# ---------------------------------------------------------------------------------------------- estimation.jl:93-220
# jacobsen and quinn: one transform, ABS2ARGMAX and a 64-byte peak record; per quinn iteration one pass over the signal that leaves a record of a few
# Float64 sums (mdsp_quinn_*; the filtered signal is never stored).  esprit is not accelerated (a dense SVD).
const EST_SUM, EST_ABS2ARGMAX = Cint(0), Cint(1)

function est_reduce_geometry(inner::Integer, len::Integer, outer::Integer, op::Integer, ::Type{T}; segments::Integer=0) where {T}
    route, S, seglen, depth, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_est_reduce_geometry_for, lib), Cint, (Int64, Int64, Int64, Cint, Cint, Int64, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                inner, len, outer, op, mdtype(T), segments, route, S, seglen, depth, ws))
    (route=Int(route[]), segments=Int(S[]), seglen=Int(seglen[]), depth=Int(depth[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code: Float64 sums (1 per real line, 2 per complex line) or Int64 (index, flag)
function est_reduce_emulate(x::Array{T}, inner::Integer, len::Integer, outer::Integer, op::Integer; segments::Integer=0, phase::Integer=0) where {T}
    words = (op == EST_SUM && T <: Real) ? 1 : 2
    out = op == EST_ABS2ARGMAX ? zeros(Int64, words, inner * outer) : zeros(Float64, words, inner * outer)
    reached = Ref{Int64}(0)
    GC.@preserve x out check(ccall((:mdsp_est_reduce_emulate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Int64, Int64, Ref{Int64}),
                                   pointer(x), pointer(out), inner, len, outer, op, mdtype(T), segments, phase, reached))
    out, Int(reached[])
end
function est_reduce_exec!(out::DeviceArray, x::DeviceArray{T}, inner::Integer, len::Integer, outer::Integer, op::Integer; segments::Integer=0) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_est_reduce_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Cint, Cint, Int64), h, inner, len, outer, op, mdtype(T), segments))
    try
        route, S, seglen, depth, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_est_reduce_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], route, S, seglen, depth, ws))
        check(ccall((:mdsp_est_reduce_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], x.ptr, out.ptr, C_NULL))
    finally
        ccall((:mdsp_est_reduce_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    out
end
# the peak record on the host, from host bins and an (index, flag) pair: the text of the device's gather
function est_peak_emulate(bins::Vector{T}, n::Integer, onesided::Bool, argmax::Vector{Int64}) where {T<:Union{ComplexF32,ComplexF64}}
    out = zeros(Int64, 8)
    GC.@preserve bins argmax out check(ccall((:mdsp_est_peak_emulate, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                                             pointer(bins), length(bins), n, onesided, mdtype(T), pointer(argmax), pointer(out)))
    out
end

# jacobsen(x, Fs)   :93-115.  Half a spectrum is enough for a real signal: a peak in the upper half gives the same value after abs.
function jacobsen(x::AbstractVector{T}, Fs::Real=1.0) where {T<:Number}
    N = length(x)
    N >= 2 || throw(ArgumentError("jacobsen: at least two samples are needed (got $N)"))
    onesided = T <: Real
    X = stft(x, N, 0; nfft=N, window=nothing, onesided=onesided)
    bins = X isa DeviceArray ? X : upload(vec(Array(X)))
    rec = DeviceArray{Int64}((10,))                              # (index, flag), then the 64-byte peak record
    est_reduce_exec!(rec, bins, 1, length(bins), 1, EST_ABS2ARGMAX)
    check(ccall((:mdsp_est_peak_gather, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                bins.ptr, length(bins), N, onesided, mdtype(eltype(bins)), rec.ptr, rec.ptr + 16, C_NULL))
    r = download(rec)
    k, flag = r[3], r[4]
    (flag != 0 || k < 0) && return NaN
    Xm, X0, Xp = reinterpret(ComplexF64, r[5:10])
    fpeak = (k < (N + 1) >> 1 ? k : k - N) * (Fs / N)           # fftfreq(N, Fs)[k + 1]
    δ = -real((Xp - Xm) / (2X0 - Xm - Xp))                       # :108
    estimate = fpeak + δ * Fs / N
    onesided ? abs(estimate) : estimate
end

function quinn_geometry(::Type{T}, n::Integer; segments::Integer=0) where {T}
    S, seglen, tile, run, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_quinn_geometry_for, lib), Cint, (Cint, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), mdtype(T), n, segments, S, seglen, tile, run, ws))
    (segments=Int(S[]), seglen=Int(seglen[]), tile=Int(tile[]), run=Int(run[]), workspace_bytes=Int(ws[]))
end
# the host emulation of one pass: {num, den, xi_1, xi_2} for a real signal (param = alpha), {re S, im S, den} for a complex one (param = omega)
function quinn_pass_emulate(x::Vector{T}, mean::Number, param::Real; segments::Integer=0) where {T}
    out = zeros(Float64, 4)
    mu = Float64[real(mean), imag(mean)]
    GC.@preserve x mu out check(ccall((:mdsp_quinn_pass_emulate_host, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
                                      pointer(x), mdtype(T), length(x), segments, pointer(mu), Float64(param), pointer(out)))
    T <: Real ? out : out[1:3]
end
function quinn_pass!(out::DeviceArray{Float64}, x::DeviceArray{T}, mean::Number, param::Real; segments::Integer=0) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_quinn_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64), h, mdtype(T), length(x), segments))
    mu = Float64[real(mean), imag(mean)]
    try
        S, seglen, tile, run, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_quinn_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], S, seglen, tile, run, ws))
        GC.@preserve mu check(ccall((:mdsp_quinn_pass_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}),
                                    h[], x.ptr, pointer(mu), Float64(param), out.ptr, C_NULL))
    finally
        ccall((:mdsp_quinn_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    out
end

# quinn(x, f0, Fs; tol, maxiters)   :157-220: the mean, the iteration and the stopping rule run in the library (mdsp_quinn_estimate)
function quinn(x::DeviceArray{T,1}, f0::Real, Fs::Real; tol=1e-6, maxiters::Integer=20) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    length(x) >= 2 || throw(ArgumentError("quinn: at least two samples are needed (got $(length(x)))"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_quinn_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64), h, mdtype(T), length(x), 0))
    est, reached, iters = Ref{Cdouble}(0), Ref{Cint}(0), Ref{Int64}(0)
    try
        check(ccall((:mdsp_quinn_estimate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Int64, Ref{Cdouble}, Ref{Cint}, Ref{Int64}, Ptr{Cvoid}),
                    h[], x.ptr, Float64(f0), Float64(Fs), Float64(tol), maxiters, est, reached, iters, C_NULL))
    finally
        ccall((:mdsp_quinn_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    est[], reached[] != 0
end
quinn(x::AbstractVector{T}, f0::Real, Fs::Real; kwargs...) where {T<:Number} = quinn(upload(convert(Vector{fftintype(T)}, x)), f0, Fs; kwargs...)
quinn(x::AbstractVector; kwargs...) = quinn(x, jacobsen(x, 1.0), 1.0; kwargs...)              # :153
quinn(x::AbstractVector, Fs::Real; kwargs...) = quinn(x, jacobsen(x, Fs), Fs; kwargs...)      # :155

# ---------------------------------------------------------------------------------------------- lpc.jl:28-159
# arburg / lpc(x, p, LPCBurg()): Burg's lattice passes on the device (mdsp_burg_*: two work arrays that do not move, 2 p launches, one copy of the
# record); levinson is host code on p + 1 numbers; lpc(x, p, LPCLevinson()) is the device xcorr followed by levinson.
struct LPCBurg end
struct LPCLevinson end

function burg_geometry(::Type{T}, n::Integer; segments::Integer=0) where {T}
    S, seglen, tile, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_burg_geometry_for, lib), Cint, (Cint, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), mdtype(T), n, segments, S, seglen, tile, ws))
    (segments=Int(S[]), seglen=Int(seglen[]), tile=Int(tile[]), workspace_bytes=Int(ws[]))
end
# the record: a (p + 1), the reflection coefficients (p), prediction_err in the real part of the last element
burg_split(rec::Vector{T}, p::Integer) where {T} = (rec[1:p+1], real(rec[2p+2]), rec[p+2:2p+1])
# the host emulation of the device code
function burg_emulate(x::Vector{T}, p::Integer; segments::Integer=0) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    rec = zeros(T, 2p + 2)
    GC.@preserve x rec check(ccall((:mdsp_burg_emulate_host, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Cvoid}),
                                   pointer(x), mdtype(T), length(x), segments, p, pointer(rec)))
    burg_split(rec, p)
end
# Burg's recursion of order p on a device vector into a device record of 2p + 2 elements; returns the cut the plan ran with
function burg_exec!(rec::DeviceArray{T}, x::DeviceArray{T,1}, p::Integer; segments::Integer=0) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_burg_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64), h, mdtype(T), length(x), segments))
    try
        S, seglen, tile, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_burg_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], S, seglen, tile, ws))
        check(ccall((:mdsp_burg_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}), h[], x.ptr, p, rec.ptr, C_NULL))
        return (segments=Int(S[]), seglen=Int(seglen[]), tile=Int(tile[]), workspace_bytes=Int(ws[]))
    finally
        ccall((:mdsp_burg_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
end
# arburg(x, p): (a with its leading 1, prediction error, reflection coefficients).  0 <= p <= N - 1 (DSP.jl divides zero by zero at p = N)
function arburg(x::DeviceArray{T,1}, p::Integer; segments::Integer=0) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    0 <= p <= length(x) - 1 || throw(ArgumentError("arburg: the order must be in [0, N - 1] = [0, $(length(x) - 1)], got $p"))
    rec = DeviceArray{T}((2p + 2,))
    burg_exec!(rec, x, p; segments=segments)
    burg_split(download(rec), p)
end
arburg(x::AbstractVector{T}, p::Integer; kwargs...) where {T<:Number} = arburg(upload(convert(Vector{fftintype(T)}, x)), p; kwargs...)

# lpc(x, p[, LPCBurg()]): arburg without the leading 1.  Host vectors and device vectors alike.
const BurgInput = Union{AbstractVector,DeviceArray{<:Any,1}}
lpc(x::BurgInput, p::Integer, ::LPCBurg) = (res = arburg(x, p); (res[1][2:end], res[2]))
lpc(x::BurgInput, p::Integer) = lpc(x, p, LPCBurg())

# levinson(r, p): the order-p solution of the Hermitian Toeplitz system whose first column is r[1:p], by Levinson's recursion on the host in the
# promoted floating type of r: (coefficients without the leading 1, error, reflection coefficients).  A device vector is read by copying p + 1 lags.
function levinson(r::AbstractVector{<:Number}, p::Integer)
    (p >= 1 && length(r) >= p + 1) || throw(ArgumentError("levinson: p >= 1 and length(R_xx) >= p + 1 are needed"))
    W = float(eltype(r))                      # Int -> Float64, Complex{Int} -> ComplexF64, Float32 stays
    lag = W[r[i] for i in 1:p+1]              # lag[j + 1] is lag j
    coef, refl, old = zeros(W, p), zeros(W, p), zeros(W, p)
    gain = -lag[2] / lag[1]
    coef[1] = refl[1] = gain
    err = real(lag[1]) * (1 - abs2(gain))
    for order in 2:p
        copyto!(old, coef)
        acc = zero(W)                         # sum over j of lag_j coef_(order - j), no conjugate, in ascending j
        for j in 1:order-1
            acc = muladd(lag[j+1], old[order-j], acc)
        end
        gain = -(lag[order+1] + acc) / err
        for j in 1:order-1
            coef[j] = muladd(gain, conj(old[order-j]), old[j])
        end
        coef[order] = refl[order] = gain
        err *= 1 - abs2(gain)
    end
    coef, err, refl
end
levinson(r::DeviceArray{T,1}, p::Integer) where {T} = levinson(download(r)[1:min(p + 1, length(r))], p)

# lpc(x, p, LPCLevinson()): the biased autocorrelation through the device xcorr, its lags 0 .. p, then levinson on the host.  A device vector is
# downloaded first (xcorr takes host vectors and uploads them itself).
function lpc(x::AbstractVector, p::Integer, ::LPCLevinson)
    n = length(x)
    1 <= p <= n - 1 || throw(ArgumentError("lpc: the order of the Levinson method must be in [1, N - 1]"))
    full = xcorr(x; scaling=:biased)
    lags = full isa DeviceArray ? download(full) : Array(full)
    coef, err, _ = levinson(lags[n:n+p], p)
    coef, err
end
lpc(x::DeviceArray{T,1}, p::Integer, m::LPCLevinson) where {T} = lpc(download(x), p, m)

# ---------------------------------------------------------------------------------------------- estimation.jl:67-75
# esprit: the Gram matrix R = X X' of the M x (N - M + 1) Hankel matrix on the device (mdsp_hankel_gram_*: two launches, Float64 sums stored and added
# in a fixed order), then eigen(Hermitian(R)), the p leading eigenvectors, \ and eigen on the host.  The span of those eigenvectors is the span of the
# first p left singular vectors the reference takes from svd(X).
const ESPRIT_MAX_M = 1024      # a cap on the host eigenproblem and on the 16 MiB of R, not on the kernels
gramtype(::Type{T}) where {T<:Real} = Float64
gramtype(::Type{T}) where {T<:Complex} = ComplexF64

function hankel_gram_geometry(::Type{T}, n::Integer, M::Integer; segments::Integer=0) where {T}
    S, seglen, tile, group, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_hankel_gram_geometry_for, lib), Cint, (Cint, Int64, Int64, Int64, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                mdtype(T), n, M, segments, S, seglen, tile, group, ws))
    (segments=Int(S[]), seglen=Int(seglen[]), tile=Int(tile[]), lag_group=Int(group[]), workspace_bytes=Int(ws[]))
end
# the host emulation of the device code
function hankel_gram_emulate(x::Vector{T}, M::Integer; segments::Integer=0) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    R = zeros(gramtype(T), M, M)
    GC.@preserve x R check(ccall((:mdsp_hankel_gram_emulate_host, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Cvoid}, Int64),
                                 pointer(x), mdtype(T), length(x), M, segments, pointer(R), M))
    R
end
# R of a device vector as a host matrix (column-major, as the library writes it)
function hankel_gram(x::DeviceArray{T,1}, M::Integer; segments::Integer=0) where {T<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_hankel_gram_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64), h, mdtype(T), length(x), M, segments))
    try
        S, seglen, tile, group, ws = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_hankel_gram_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], S, seglen, tile, group, ws))
        R = DeviceArray{gramtype(T)}((M, M))
        check(ccall((:mdsp_hankel_gram_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), h[], x.ptr, R.ptr, M, C_NULL))
        return download(R)
    finally
        ccall((:mdsp_hankel_gram_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
end
hankel_gram(x::AbstractVector{T}, M::Integer; kwargs...) where {T<:Number} = hankel_gram(upload(convert(Vector{fftintype(T)}, x)), M; kwargs...)

# the host finish (:71-74) from the Gram matrix
function esprit_from_gram(R::AbstractMatrix, p::Integer, Fs::Real=1.0)
    all(isfinite, R) || throw(ArgumentError("esprit: the signal holds Infs or NaNs"))          # the reference's svd refuses them
    V = eigen(Hermitian(Matrix(R))).vectors                                                     # eigenvalues ascending
    U = V[:, end:-1:end-p+1]
    D = eigen(U[1:end-1, :] \ U[2:end, :]).values
    Float64.(angle.(D) .* (Fs / 2π))
end

# esprit(x, M, p, Fs=1.0).  p < 1 or M > N: ArgumentError (a BoundsError in DSP.jl); p >= M, 2M - 1 > N, M > ESPRIT_MAX_M: UnsupportedError
function esprit(x::Union{AbstractArray{<:Number},DeviceArray}, M::Integer, p::Integer, Fs::Real=1.0)
    count(!isone, size(x)) <= 1 || throw(ArgumentError("`x` must be a 1D signal"))              # :68
    N = length(x)
    (p >= 1 && 1 <= M <= N) || throw(ArgumentError("esprit: p >= 1 and 1 <= M <= N are needed (M = $M, p = $p, N = $N)"))
    p < M || throw(UnsupportedError("esprit: p < M is needed (M = $M, p = $p)"))
    2M - 1 <= N || throw(UnsupportedError("esprit: 2 M - 1 <= N is needed (M = $M, N = $N)"))
    M <= ESPRIT_MAX_M || throw(UnsupportedError("esprit: M <= $ESPRIT_MAX_M is needed (got $M)"))
    v = x isa DeviceArray ? (ndims(x) == 1 ? x : upload(vec(download(x)))) : vec(collect(x))
    esprit_from_gram(hankel_gram(v, M), p, Fs)
end

function shift_geometry(l::Integer, s::Integer, elem_bytes::Integer, in_place::Bool; tile::Integer=0, route::Integer=SHIFT_AUTO)
    r, t, c, n, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_shift_geometry_for, lib), Cint, (Int64, Int64, Int64, Cint, Int64, Cint, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                l, s, elem_bytes, in_place, tile, route, r, t, c, n, ws))
    (route=Int(r[]), tile=Int(t[]), chunk=Int(c[]), ntiles=Int(n[]), workspace_bytes=Int(ws[]))
end
# the host walk of a plan's launches (units of a launch in three orders): (result, reads that came after a write)
function shift_emulate(x::Vector{T}, s::Integer; tile::Integer=0, route::Integer=SHIFT_AUTO, order::Integer=0, in_place::Bool=true) where {T}
    src = copy(x)
    dst = in_place ? src : similar(x)
    bad = Ref{Int64}(0)
    GC.@preserve src dst check(ccall((:mdsp_shift_emulate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Cint, Cint, Ref{Int64}),
                                     pointer(src), pointer(dst), length(x), s, sizeof(T), tile, route, order, bad))
    dst, Int(bad[])
end
function _shift!(y::DeviceArray{T,1}, x::DeviceArray{T,1}, s::Integer; tile::Integer=0, route::Integer=SHIFT_AUTO) where {T}
    l = length(x)
    abs(s) > l && throw(DomainError(s, "The absolute value of s must not be greater than the length of x"))      # :359-361
    sizeof(T) in (4, 8, 16) || throw(UnsupportedError("shiftsignal: elements of $(sizeof(T)) bytes are not accelerated"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_shift_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Cint, Int64, Cint), h, l, s, sizeof(T), x.ptr == y.ptr, tile, route))
    try
        r, t, c, n, ws = Ref{Cint}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:mdsp_shift_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}), h[], r, t, c, n, ws))
        check(ccall((:mdsp_shift_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], x.ptr, y.ptr, C_NULL))
    finally
        ccall((:mdsp_shift_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
    y
end
# shiftsignal!(x, s) / shiftsignal(x, s)   :357-395
shiftsignal!(x::DeviceArray{T,1}, s::Integer; kwargs...) where {T} = _shift!(x, x, s; kwargs...)
shiftsignal(x::DeviceArray{T,1}, s::Integer; kwargs...) where {T} = _shift!(DeviceArray{T}(size(x)), x, s; kwargs...)
shiftsignal(x::AbstractVector, s::Integer; kwargs...) = download(shiftsignal!(upload(Array(x)), s; kwargs...))
shiftsignal!(x::AbstractVector, s::Integer; kwargs...) = copyto!(x, shiftsignal(x, s; kwargs...))
# alignsignals!(x, y) / alignsignals(x, y)   :404-430
function alignsignals!(x, y)
    d = finddelay(x isa DeviceArray ? download(x) : x, y isa DeviceArray ? download(y) : y)
    shiftsignal!(x, -d), d
end
function alignsignals(x, y)
    d = finddelay(x isa DeviceArray ? download(x) : x, y isa DeviceArray ? download(y) : y)
    shiftsignal(x, -d), d
end

# ---------------------------------------------------------------------------------------------- periodograms
# result types   periodograms.jl:262-330, :765-793
abstract type TFR{T} end
struct Periodogram{T,F<:AbstractVector,V<:AbstractVector{T}} <: TFR{T}
    power::V
    freq::F
end
struct Spectrogram{T,F<:AbstractVector,M<:AbstractMatrix{T}} <: TFR{T}
    power::M
    freq::F
    time::StepRangeLen{Float64,Base.TwicePrecision{Float64},Base.TwicePrecision{Float64}}
end
power(p::TFR) = p.power
freq(p::TFR) = p.freq
Base.time(p::Spectrogram) = p.time
# AbstractFFTs.rfftfreq / fftfreq (the reference's `freq` fields are AbstractFFTs.Frequencies; these are the same values)
rfftfreq(n::Integer, fs::Real=1) = (0:(n >> 1)) .* (fs / n)
fftfreq(n::Integer, fs::Real=1) = vcat(0:((n - 1) >> 1), -(n >> 1):-1) .* (fs / n)

compute_window(::Nothing, n::Int) = (nothing, Float64(n))                               # periodograms.jl:248-257
function compute_window(window::Function, n::Int)
    win = window(n)::Vector{Float64}
    (win, sum(abs2, win))
end
function compute_window(window::AbstractVector, n::Int)
    length(window) == n || throw(DimensionMismatch("length of window must match input"))
    w = convert(Vector{Float64}, window)
    (w, sum(abs2, w))
end
winptr(::Nothing) = Ptr{Cdouble}(C_NULL)
winptr(w::Vector{Float64}) = pointer(w)

# arraysplit(s, n, noverlap, nfft = n, window = nothing)   periodograms.jl:32-137: frame k = s[(k-1)(n-noverlap)+1 ...] .* window, zero
# padded to nfft.  The frames are materialised on the device by the library's framer (what the fused kernels do on the fly; bit-exact
# with the reference, tests/test_gpu_parity.py::test_frames_bit_exact) and indexed like the reference's ArraySplit.
struct ArraySplit{T} <: AbstractVector{Vector{T}}
    frames::Matrix{T}
end
Base.size(a::ArraySplit) = (size(a.frames, 2),)
Base.getindex(a::ArraySplit, k::Int) = a.frames[:, k]
function arraysplit(s::AbstractVector{T}, n::Integer, noverlap::Integer, nfft::Integer=n, window=nothing) where {T<:Number}
    (0 <= noverlap < n) || throw(DomainError((; noverlap, n), "noverlap must be between zero and n"))       # :44
    nfft >= n || throw(DomainError((; nfft, n), "nfft must be >= n"))                                         # :45
    S = fftintype(T)
    win, _ = compute_window(window, Int(n))
    sd = todevice(s, S)
    k = framecount(length(s), n, noverlap)
    out = DeviceArray{S}((Int(nfft), k))
    GC.@preserve win (k > 0 && check(ccall((:mdsp_frames, lib), Cint,
        (Ptr{Cvoid}, Int64, Cint, Int64, Int64, Int64, Ptr{Cdouble}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        sd.ptr, length(s), mdtype(S), n, noverlap, nfft, winptr(win), 0, k, out.ptr, C_NULL)))
    ArraySplit{S}(download(out))
end

mutable struct WelchConfig                                                                        # periodograms.jl:516-587
    h::Ptr{Cvoid}
    borrowed::Bool
    nsamples::Int; noverlap::Int; onesided::Bool; nfft::Int; fs::Float64
    freq::AbstractVector; window; r::Float64; intype::DataType; nout::Int
end
function WelchConfig(nsamples, ::Type{T}; n::Int=nsamples >> 3, noverlap::Int=n >> 1, onesided::Bool=T <: Real,
                     nfft::Int=nextfastfft(n), fs::Real=1, window=nothing, engine=ENGINE_AUTO, cached::Bool=false) where {T}
    onesided && T <: Complex && throw(ArgumentError("cannot compute one-sided FFT of a complex signal"))
    nfft >= n || throw(DomainError((; nfft, n), "nfft must be >= n"))
    win, norm2 = compute_window(window, n)
    r = fs * norm2
    S = fftintype(T)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    if cached   # the function-style welch_pgram(s, n, noverlap): plan from the library's LRU, borrowed
        GC.@preserve win check(ccall((:mdsp_welch_plan_cached, lib), Cint,
            (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ptr{Cdouble}, Cdouble, Cint, Cint, Cint, Ptr{Cvoid}),
            p, n, noverlap, nfft, winptr(win), r, onesided, mdtype(S), engine, C_NULL))
    else
        GC.@preserve win check(ccall((:mdsp_welch_plan_create, lib), Cint,
            (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ptr{Cdouble}, Cdouble, Cint, Cint, Cint),
            p, n, noverlap, nfft, winptr(win), r, onesided, mdtype(S), engine))
    end
    no, eng = Ref{Int64}(0), Ref{Cint}(0)
    check(ccall((:mdsp_welch_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Cint}), p[], no, eng))
    cfg = WelchConfig(p[], cached, n, noverlap, onesided, nfft, fs, onesided ? rfftfreq(nfft, fs) : fftfreq(nfft, fs), win, r, S, Int(no[]))
    cached || finalizer(x -> ccall((:mdsp_welch_plan_destroy, lib), Cint, (Ptr{Cvoid},), x.h), cfg)
    cfg
end
WelchConfig(data::AbstractArray; kw...) = WelchConfig(size(data, 1), eltype(data); kw...)

# welch_pgram(s, config) -> Periodogram   periodograms.jl:702-705, :746-759.  Columns of a matrix are channels (`power` is then a matrix).
function welch_power(s::DeviceArray{T}, config::WelchConfig) where {T}
    len = size(s, 1); nch = ncolumns(s)
    out = DeviceArray{fftabs2type(config.intype)}(ndims(s) == 1 ? (config.nout,) : (config.nout, nch))
    check(ccall((:mdsp_welch_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                config.h, s.ptr, len, nch, len, out.ptr, config.nout, C_NULL))
    out
end
# Host Arrays: mdsp_welch_exec_host (time chunks of whole frames through the pipeline; Float64 sums accumulate in the plan)
function welch_power(s::Array{T}, config::WelchConfig; pinned::Bool=false) where {T}
    len = size(s, 1); nch = ncolumns(s)
    out = Array{fftabs2type(T)}(undef, ndims(s) == 1 ? (config.nout,) : (config.nout, nch))
    GC.@preserve s out check(ccall((:mdsp_welch_exec_host, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Cint),
                                   config.h, pointer(s), len, nch, len, pointer(out), config.nout, pinned ? HOST_PINNED : Cint(0)))
    out
end
function welch_pgram(s::Union{AbstractVecOrMat{T},DeviceArray{T}}, config::WelchConfig; kw...) where {T<:Number}
    fftintype(T) == config.intype ||
        throw(ArgumentError("float(eltype(s)) = $T doesn't match the eltype of the input buffer: $(config.intype)."))
    p = s isa DeviceArray ? welch_power(s, config) : welch_power(convert(Array{config.intype}, s), config; kw...)
    ndims(p) == 1 ? Periodogram(p isa DeviceArray ? download(p) : p, config.freq) : (power = p, freq = config.freq)
end
welch_pgram(s::AbstractVector, n::Int=length(s) >> 3, noverlap::Int=n >> 1; kw...) =
    welch_pgram(s, WelchConfig(s; n, noverlap, cached=true, kw...))
function welch_pgram!(out::AbstractVector, s::AbstractVector{T}, config::WelchConfig) where {T<:Number}        # periodograms.jl:734-744
    length(out) == length(config.freq) || throw(DimensionMismatch("Expected `output` to be of length `length(config.freq)`; got `length(output)` = $(length(out)) and `length(config.freq)` = $(length(config.freq))"))
    eltype(out) == fftabs2type(T) || throw(ArgumentError("Eltype of output ($(eltype(out))) doesn't match the expected type: $(fftabs2type(T))."))
    float(T) == config.intype || throw(ArgumentError("float(eltype(s)) = $T doesn't match the eltype of the input buffer: $(config.intype)."))
    copyto!(out, power(welch_pgram(s, config)))
    Periodogram(out, config.freq)
end
welch_pgram!(out::AbstractVector, s::AbstractVector, n::Int=length(s) >> 3, noverlap::Int=n >> 1; kw...) =
    welch_pgram!(out, s, WelchConfig(s; n, noverlap, cached=true, kw...))

# Streaming form (mdsp_welch_exec IS reset + accumulate + finalize): a stream handed over slice by slice -- each slice whole frames,
# consecutive slices overlapping by n - hop samples -- or by several ranks (welch_allreduce!).   periodograms.jl:746-759
welch_reset!(c::WelchConfig) = (check(ccall((:mdsp_welch_reset, lib), Cint, (Ptr{Cvoid},), c.h)); c)
function welch_accumulate!(c::WelchConfig, s::DeviceArray)
    len = size(s, 1)
    check(ccall((:mdsp_welch_accumulate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}), c.h, s.ptr, len, ncolumns(s), len, C_NULL))
    c
end
function welch_frames_accumulated(c::WelchConfig)
    k = Ref{Int64}(0)
    check(ccall((:mdsp_welch_frames_accumulated, lib), Cint, (Ptr{Cvoid}, Ref{Int64}), c.h, k)); Int(k[])
end
# the Float64 accumulator itself (device pointer, element count): what a caller-side collective (MPI.jl ...) would sum over ranks
function welch_accumulator(c::WelchConfig)
    p, n = Ref{Ptr{Cvoid}}(C_NULL), Ref{Int64}(0)
    check(ccall((:mdsp_welch_accumulator, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), c.h, p, n))
    (ptr = p[], count = Int(n[]))
end
function welch_finalize(c::WelchConfig, nch::Integer=1; frames_total::Integer=0)
    out = DeviceArray{fftabs2type(c.intype)}((c.nout, Int(nch)))
    check(ccall((:mdsp_welch_finalize, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}), c.h, frames_total, out.ptr, c.nout, C_NULL))
    out
end

# ---------------------------------------------------------------------------------------------- multi-GPU (one process per GPU)
# The reference loops over columns / channels serially (Filters/filt.jl:504; `mapslices` stream_filt.jl:768).  Here rank r owns a
# contiguous block of channels and runs the single-GPU methods on them; the ONLY collective is the all-reduce of an nout-value PSD for
# the cross-channel Welch mean -- RCCL over xGMI, behind the C ABI.  Bootstrap: rank 0 makes the 128-byte id, the host ships it
# (e.g. `MPI.Bcast!(id, 0, comm)` or a shared file), every rank calls Comm(id, rank, nranks) after init(device).
mutable struct Comm
    h::Ptr{Cvoid}
    rank::Int
    nranks::Int
end
function unique_id()
    id = Vector{UInt8}(undef, 128)
    GC.@preserve id check(ccall((:mdsp_comm_unique_id, lib), Cint, (Ptr{Cvoid},), pointer(id)))
    id
end
function Comm(id::Vector{UInt8}, rank::Integer, nranks::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve id check(ccall((:mdsp_comm_init_rank, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Cint, Cint), p, pointer(id), rank, nranks))
    r, n = Ref{Cint}(-1), Ref{Cint}(-1)
    check(ccall((:mdsp_comm_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), p[], r, n))
    c = Comm(p[], Int(r[]), Int(n[]))
    finalizer(x -> ccall((:mdsp_comm_destroy, lib), Cint, (Ptr{Cvoid},), x.h), c)
    c
end
channel_shard(nch::Integer, rank::Integer, nranks::Integer) = (per = cld(nch, nranks); (min(rank * per, nch) + 1):min((rank + 1) * per, nch))
# in-place sum over ranks of a device array (the bare transport)
function allreduce_sum!(x::DeviceArray{T}, comm::Comm) where {T<:Union{Float32,Float64}}
    check(ccall((:mdsp_allreduce_sum, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}), comm.h, x.ptr, length(x), mdtype(T), C_NULL)); x
end
# sum over this rank's channels (columns) of a (len, nch) device matrix
function channel_sum(x::DeviceArray{T}) where {T<:Union{Float32,Float64}}
    len = size(x, 1)
    out = DeviceArray{T}((len,))
    check(ccall((:mdsp_channel_sum, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}), x.ptr, len, ncolumns(x), len, mdtype(T), out.ptr, C_NULL))
    out
end

# mean over ALL channels (across ranks) of the per-channel Welch PSDs: local sum on the device -> ncclAllReduce(sum) of nout values ->
# 1/nch_total, one C-ABI call.  `s`: this rank's channels as columns.
function welch_channel_mean(s::DeviceArray{T}, config::WelchConfig, nch_total::Integer, comm::Union{Comm,Nothing}=nothing) where {T}
    len = size(s, 1); nloc = ncolumns(s)
    R = fftabs2type(config.intype)
    psd = DeviceArray{R}((config.nout, max(nloc, 1)))
    nloc > 0 && check(ccall((:mdsp_welch_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                            config.h, s.ptr, len, nloc, len, psd.ptr, config.nout, C_NULL))
    mean = DeviceArray{R}((config.nout,))
    check(ccall((:mdsp_welch_mean_allreduce, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                config.h, psd.ptr, nloc, config.nout, nch_total, mean.ptr, comm === nothing ? C_NULL : comm.h, C_NULL))
    mean
end
# one stream split along time over ranks: after welch_accumulate! on every rank's slice, sum the Float64 accumulators and frame counts
welch_allreduce!(c::WelchConfig, comm::Comm) =
    (check(ccall((:mdsp_welch_allreduce, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.h, comm.h, C_NULL)); c)

# ---------------------------------------------------------------------------------------------- stft / spectrogram / periodogram
# periodograms.jl:872-897, :828-837, :393-417.  The plan (window upload, tables, transforms) comes from the library's LRU: the reference
# builds its FFTW plan on every call, here a call costs ~90 us instead of ~370.
function stft_plan(n, noverlap, nfft, win, r, onesided::Bool, psdonly::Bool, ::Type{S}, engine) where {S}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve win check(ccall((:mdsp_stft_plan_cached, lib), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ptr{Cdouble}, Cdouble, Cint, Cint, Cint, Cint, Ptr{Cvoid}),
        p, n, noverlap, nfft, winptr(win), r, onesided, psdonly, mdtype(S), engine, C_NULL))
    no, eng = Ref{Int64}(0), Ref{Cint}(0)
    check(ccall((:mdsp_stft_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Cint}), p[], no, eng))
    (p[], Int(no[]))
end
# an owned plan (mdsp_stft_plan_create / _destroy) for callers that keep one across many calls
mutable struct StftPlan
    h::Ptr{Cvoid}
    function StftPlan(n, noverlap, nfft, win, r, onesided::Bool, psdonly::Bool, ::Type{S}, engine=ENGINE_AUTO) where {S}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve win check(ccall((:mdsp_stft_plan_create, lib), Cint,
            (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Ptr{Cdouble}, Cdouble, Cint, Cint, Cint, Cint),
            p, n, noverlap, nfft, winptr(win), r, onesided, psdonly, mdtype(S), engine))
        o = new(p[])
        finalizer(x -> ccall((:mdsp_stft_plan_destroy, lib), Cint, (Ptr{Cvoid},), x.h), o)
        o
    end
end
# the kernel family a Welch (kind 0) or STFT / multitaper (kind 1) plan of this size would record, without a plan or a device (route: MDSP_ROUTE_* of
# include/mi355dsp.h; r0: the column factor of the R0 x row routes, else 0)
function spectral_route_for(kind::Integer, ::Type{T}, nfft::Integer, engine::Integer=ENGINE_AUTO) where {T}
    eng, route, r0 = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:mdsp_spectral_route_for, lib), Cint, (Cint, Cint, Int64, Cint, Ref{Cint}, Ref{Cint}, Ref{Cint}), kind, mdtype(T), nfft, engine, eng, route, r0))
    (engine = Int(eng[]), route = Int(route[]), r0 = Int(r0[]))
end
# how many of `units` units the chunked engine loop `kind` (MDSP_CHUNK_* of include/mi355dsp.h) takes per chunk under the current tunables; no device
function chunk_units_for(kind::Integer, ::Type{T}, n::Integer, units::Integer) where {T}
    c = Ref{Int64}(0)
    check(ccall((:mdsp_chunk_units_for, lib), Cint, (Cint, Cint, Int64, Int64, Ref{Int64}), kind, mdtype(T), n, units, c))
    Int(c[])
end
function stft(s::Union{AbstractVecOrMat{T},DeviceArray{T}}, n::Int=size(s, 1) >> 3, noverlap::Int=n >> 1, psdonly::Bool=false;
              onesided::Bool=T <: Real, nfft::Int=nextfastfft(n), fs::Real=1, window=nothing, engine=ENGINE_AUTO, pinned::Bool=false) where {T}
    onesided && T <: Complex && throw(ArgumentError("cannot compute one-sided FFT of a complex signal"))
    win, norm2 = compute_window(window, n)
    (0 ≤ noverlap < n) || throw(DomainError((; noverlap, n), "noverlap must be between zero and n"))
    nfft >= n || throw(DomainError((; nfft, n), "nfft must be >= n"))
    S = fftintype(T)
    plan, nout = stft_plan(n, noverlap, nfft, win, fs * norm2, onesided, psdonly, S, engine)
    len = size(s, 1); nch = ncolumns(s)
    k = framecount(len, n, noverlap)
    O = psdonly ? fftabs2type(S) : fftouttype(S)
    dims = ndims(s) == 1 ? (nout, k) : (nout, k, nch)
    if s isa DeviceArray
        sd = todevice(s, S)
        out = DeviceArray{O}(dims)
        k > 0 && check(ccall((:mdsp_stft_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                             plan, sd.ptr, len, nch, len, out.ptr, nout, nout * k, C_NULL))
        return out
    end
    # host Arrays: mdsp_stft_exec_host -- the output (2-8x the input) never lives on the device whole
    sh = convert(Array{S}, s)
    out = zeros(O, dims)
    GC.@preserve sh out (k > 0 && check(ccall((:mdsp_stft_exec_host, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Cint),
                                              plan, pointer(sh), len, nch, len, pointer(out), nout, nout * k, pinned ? HOST_PINNED : Cint(0))))
    out
end
function spectrogram(s::AbstractVector{T}, n::Int=length(s) >> 3, noverlap::Int=n >> 1; onesided::Bool=T <: Real,
                     nfft::Int=nextfastfft(n), fs::Real=1, window=nothing) where {T}
    out = stft(s, n, noverlap, true; onesided, nfft, fs, window)
    Spectrogram(out, onesided ? rfftfreq(nfft, fs) : fftfreq(nfft, fs),
                (n / 2 : n - noverlap : (size(out, 2) - 1) * (n - noverlap) + n / 2) / fs)                    # :835
end
function periodogram(s::AbstractVector{T}; onesided::Bool=T <: Real, nfft::Int=nextfastfft(length(s)), fs::Real=1, window=nothing) where {T}
    onesided && T <: Complex && throw(ArgumentError("cannot compute one-sided FFT of a complex signal"))     # :396
    nfft >= length(s) || throw(DomainError((; nfft, n=length(s)), "nfft must be >= n = length(s)"))        # :397
    p = stft(s, length(s), 0, true; onesided, nfft, fs, window)
    Periodogram(vec(p), onesided ? rfftfreq(nfft, fs) : fftfreq(nfft, fs))
end

# 2-D periodogram   periodograms.jl:284-288 (Periodogram2), :330-339 (freq, fftshift), :473-509 (periodogram of a real matrix)
struct Periodogram2{T,F1<:AbstractVector,F2<:AbstractVector,M<:AbstractMatrix{T}} <: TFR{T}
    power::M
    freq1::F1
    freq2::F2
end
freq(p::Periodogram2) = (p.freq1, p.freq2)
# the reference's three methods: both dimensions shift when freq1 is two-sided (fftfreq), only dimension 2 when freq1 is not
twosided(f::AbstractVector) = length(f) > 1 && any(<(0), diff(f))
shifted(f::AbstractVector) = circshift(f, length(f) >> 1)
function fftshift(p::Periodogram2)
    twosided(p.freq1) && return Periodogram2(circshift(p.power, size(p.power) .>> 1), shifted(p.freq1), twosided(p.freq2) ? shifted(p.freq2) : p.freq2)
    twosided(p.freq2) && return Periodogram2(circshift(p.power, (0, size(p.power, 2) >> 1)), p.freq1, shifted(p.freq2))
    p
end
# kmax, the wave counts and the number of radial row partials for nfft (host arithmetic, no device)
function periodogram2_geometry(nfft::NTuple{2,Int})
    kmax, parts = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_periodogram2_geometry_for, lib), Cint, (Int64, Int64, Ref{Int64}, Ptr{Int64}, Ref{Int64}), nfft[1], nfft[2], kmax, C_NULL, parts))
    wc = zeros(Int64, kmax[])
    check(ccall((:mdsp_periodogram2_geometry_for, lib), Cint, (Int64, Int64, Ref{Int64}, Ptr{Int64}, Ref{Int64}), nfft[1], nfft[2], kmax, wc, parts))
    (Int(kmax[]), wc, Int(parts[]))
end
function periodogram(s::Union{AbstractMatrix{T},DeviceArray{T,2}}; nfft::NTuple{2,Int}=nextfastfft.(size(s)), fs::Real=1,
                     radialsum::Bool=false, radialavg::Bool=false, engine=ENGINE_AUTO) where {T<:Real}
    n1, n2 = size(s)
    n1 <= nfft[1] && n2 <= nfft[2] || throw(ArgumentError("nfft must be >= size(s)"))                     # :477
    n1 > 1 && n2 > 1 || throw(ArgumentError("dimensions of s must be > 1"))                               # :478
    radialsum && radialavg && throw(ArgumentError("radialsum and radialavg are mutually exclusive"))      # :480
    ptype = radialsum ? 1 : radialavg ? 2 : 0
    S = fftintype(T)
    O = fftabs2type(S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mdsp_periodogram2_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Int64, Cdouble, Cint, Cint, Cint),
                h, n1, n2, nfft[1], nfft[2], fs, ptype, mdtype(S), engine))
    try
        nout, ws, eng = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
        check(ccall((:mdsp_periodogram2_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}), h[], nout, ws, eng))
        sd = todevice(s, S)
        out = ptype == 0 ? DeviceArray{O}(nfft) : DeviceArray{O}((Int(nout[]),))
        check(ccall((:mdsp_periodogram2_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                    h[], sd.ptr, n1, out.ptr, nfft[1], C_NULL))
        power = download(out)          # the result types hold host arrays (as welch_pgram's Periodogram)
        ptype == 0 && return Periodogram2(power, fftfreq(nfft[1], fs), fftfreq(nfft[2], fs))
        Periodogram(power, (0:Int(nout[]) - 1) .* (fs / minimum(nfft)))
    finally
        ccall((:mdsp_periodogram2_plan_destroy, lib), Cint, (Ptr{Cvoid},), h[])
    end
end

# ---------------------------------------------------------------------------------------------- filter design needed as INPUTS of the path
# kaiserord / Kaiser window / windowed-sinc low-pass / resample_filter   Filters/design.jl:547-559, :235-240, :598-602, :683-720; windows.jl
function kaiserord(transitionwidth::Real, attenuation::Real=60)
    n = ceil(Int, (attenuation - 7.95) / (π * 2.285 * transitionwidth)) + 1
    β = attenuation > 50 ? 0.1102 * (attenuation - 8.7) :
        attenuation >= 21 ? 0.5842 * (attenuation - 21)^0.4 + 0.07886 * (attenuation - 21) : 0.0
    (n, β / π)
end
function besseli0(x::Float64)          # power series of the modified Bessel function I0 (enough for Kaiser windows: |x| < 50)
    s = t = 1.0
    for k in 1:200
        t *= (x / (2k))^2
        s += t
        t < eps(s) && break
    end
    s
end
kaiser(n::Integer, α::Real) = n == 1 ? [1.0] : [besseli0(π * α * sqrt(1 - (2 * (k - 1) / (n - 1) - 1)^2)) / besseli0(π * α) for k in 1:n]
function lowpass_firwindow(w::Real, window::Vector{Float64}; fs::Real=2, scale::Bool=true)
    w > 0 || throw(DomainError(w, "frequencies must be positive"))
    f = 2 * w / fs
    f < 1 || throw(DomainError(w, "frequencies must be less than the Nyquist frequency"))
    n = length(window)
    sincn(x) = x == 0 ? 1.0 : sin(π * x) / (π * x)
    taps = [f * sincn(f * (k - (n + 1) / 2)) * window[k] for k in 1:n]
    scale ? taps ./ sum(taps) : taps
end
function resample_filter(rate::AbstractFloat, Nϕ::Integer=32, rel_bw::Real=1.0, attenuation::Real=60)        # design.jl:683-702
    f_nyq = rate >= 1.0 ? 1.0 / Nϕ : rate / Nϕ
    cutoff = f_nyq * rel_bw
    hLen, α = kaiserord(cutoff * 0.2, attenuation)
    hLen = Nϕ * ceil(Int, hLen / Nϕ)
    iseven(hLen) && (hLen += 1)
    lowpass_firwindow(cutoff, kaiser(hLen, α)) .* Nϕ
end
function resample_filter(rate::Union{Integer,Rational}, rel_bw::Real=1.0, attenuation::Real=60)               # design.jl:704-720
    Nϕ = numerator(rate)
    f_nyq = min(1 / Nϕ, 1 / denominator(rate))
    cutoff = f_nyq * rel_bw
    hLen, α = kaiserord(cutoff * 0.2, attenuation)
    hLen = Nϕ * ceil(Int, hLen / Nϕ)
    iseven(hLen) && (hLen += 1)
    lowpass_firwindow(cutoff, kaiser(hLen, α)) .* Nϕ
end

# ---------------------------------------------------------------------------------------------- FIRFilter / resample
mutable struct FIRFilter                                                                 # stream_filt.jl:137-178
    h::Ptr{Cvoid}
    taps::Vector
    ratio::Rational{Int}
    xtype::DataType
    nch::Int
end
# exact=true: the generic kernel only -- every output reads exactly its own tapsPerϕ-sample window, so NaN / Inf samples leave exactly DSP.jl's hole
# complex taps (ComplexF32 / ComplexF64) are multiplied as they are, no conjugate; the output is promote_type(Th, xtype)
function FIRFilter(taps::Vector{Th}, ratio::Union{Integer,Rational}=1; xtype::DataType=Th, nch::Integer=1, exact::Bool=false) where {Th<:Union{Float32,Float64,ComplexF32,ComplexF64}}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    r = convert(Rational{Int}, ratio)
    GC.@preserve taps check(ccall((:mdsp_fir_create, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cint, Int64),
                                  p, pointer(taps), length(taps), numerator(r), denominator(r), mdtype(Th), mdtype(xtype), nch))
    exact && check(ccall((:mdsp_fir_set_exact, lib), Cint, (Ptr{Cvoid}, Cint), p[], 1))
    f = FIRFilter(p[], taps, r, xtype, nch)
    finalizer(x -> ccall((:mdsp_fir_destroy, lib), Cint, (Ptr{Cvoid},), x.h), f)
    f
end
reset!(f::FIRFilter) = (check(ccall((:mdsp_fir_reset, lib), Cint, (Ptr{Cvoid},), f.h)); f)               # :247-276
setphase!(f::FIRFilter, ϕ::Real) = check(ccall((:mdsp_fir_setphase, lib), Cint, (Ptr{Cvoid}, Cdouble), f.h, ϕ))  # :216-229
function timedelay(f::FIRFilter)                                                                           # :400-403
    τ = Ref{Cdouble}(0)
    check(ccall((:mdsp_fir_timedelay, lib), Cint, (Ptr{Cvoid}, Ref{Cdouble}), f.h, τ)); τ[]
end
function firinfo(f::FIRFilter)
    kind, od = Ref{Cint}(0), Ref{Cint}(0)
    L, M, tp, hl = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_fir_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Cint}), f.h, kind, L, M, tp, hl, od))
    (kind = Int(kind[]), L = Int(L[]), M = Int(M[]), tapsPerϕ = Int(tp[]), historyLen = Int(hl[]), outtype = JLTYPE[od[] + 1])
end
# the reference's state: (ϕIdx, inputDeficit, history) with 1-based ϕIdx   stream_filt.jl:141, :59-79
function getstate(f::FIRFilter)
    hl = firinfo(f).historyLen
    hist = zeros(f.xtype, max(hl, 1), f.nch)
    ϕ, d = Ref{Int64}(0), Ref{Int64}(0)
    GC.@preserve hist check(ccall((:mdsp_fir_get_state, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}), f.h, ϕ, d, pointer(hist)))
    (ϕIdx = Int(ϕ[]), inputDeficit = Int(d[]), history = hist[1:hl, :])
end
function setstate!(f::FIRFilter, ϕIdx::Integer, inputDeficit::Integer, history::Union{Nothing,AbstractMatrix}=nothing)
    hist = history === nothing ? nothing : convert(Matrix{f.xtype}, history)
    GC.@preserve hist check(ccall((:mdsp_fir_set_state, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}), f.h, ϕIdx, inputDeficit,
                                  hist === nothing ? C_NULL : pointer(hist)))
    f
end
# which device kernel a chunk of `n` samples would take: 0 generic, 1 register-tap, 2 matrix-core (diagnostics; results do not depend on it)
function kernel_path(f::FIRFilter, n::Integer)
    p = Ref{Cint}(-1)
    check(ccall((:mdsp_fir_kernel_path, lib), Cint, (Ptr{Cvoid}, Int64, Ref{Cint}), f.h, n, p)); Int(p[])
end
# geometry of the matrix-core kernel for a filter of hlen taps at L // M (host arithmetic only; tests place their seam windows with it)
function fir_mm_geometry(L::Integer, M::Integer, hlen::Integer, ::Type{Th}, ::Type{Tx}) where {Th,Tx}
    o = zeros(Int64, 12)
    GC.@preserve o check(ccall((:mdsp_fir_mm_geometry, lib), Cint, (Int64, Int64, Int64, Cint, Cint, Ptr{Int64}), L, M, hlen, mdtype(Th), mdtype(Tx), pointer(o)))
    o
end
function outputlength(f::FIRFilter, inlen::Integer)                                                        # :324-338
    o = Ref{Int64}(0)
    check(ccall((:mdsp_fir_outputlength, lib), Cint, (Ptr{Cvoid}, Int64, Ref{Int64}), f.h, inlen, o)); Int(o[])
end
function inputlength(f::FIRFilter, outlen::Integer, r::RoundingMode=RoundDown)                             # :366-383
    o = Ref{Int64}(0)
    check(ccall((:mdsp_fir_inputlength, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ref{Int64}), f.h, outlen,
                (r == RoundUp || r == RoundFromZero) ? 1 : 0, o)); Int(o[])
end

# filt(f, x): next chunk, state carried on the device   stream_filt.jl:627-637
function filt(f::FIRFilter, x::DeviceArray)
    xd = todevice(x, f.xtype)
    xlen = size(xd, 1)
    ycap = max(outputlength(f, xlen), 0)
    y = DeviceArray{firinfo(f).outtype}(f.nch == 1 ? (ycap,) : (ycap, f.nch))
    nw = Ref{Int64}(0)
    check(ccall((:mdsp_fir_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ref{Int64}, Ptr{Cvoid}),
                f.h, xd.ptr, xlen, xlen, y.ptr, ycap, max(ycap, 1), nw, C_NULL))
    nw[] == ycap || throw(AssertionError("Length of resampled output different from expectation."))
    y
end
# host Arrays: mdsp_fir_exec_host -- the stream passes through the stateful filter in time chunks (H2D || kernel || D2H)
function filt(f::FIRFilter, x::AbstractVecOrMat; pinned::Bool=false)
    xh = convert(Array{f.xtype}, x)
    xlen = size(xh, 1)
    ycap = max(outputlength(f, xlen), 0)
    y = Array{firinfo(f).outtype}(undef, f.nch == 1 ? (ycap,) : (ycap, f.nch))
    nw = Ref{Int64}(0)
    GC.@preserve xh y check(ccall((:mdsp_fir_exec_host, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ref{Int64}, Cint),
                                  f.h, pointer(xh), xlen, xlen, pointer(y), ycap, max(ycap, 1), nw, pinned ? HOST_PINNED : Cint(0)))
    nw[] == ycap || throw(AssertionError("Length of resampled output different from expectation."))
    y
end
# stateless filt(h, x, ratio)   stream_filt.jl:663-666
filt(h::Vector, x::AbstractVector, ratio::Union{Integer,Rational}) = filt(FIRFilter(h, ratio; xtype=fftintype(eltype(x))), x)

# resample(x, rate[, h]; dims)   stream_filt.jl:688-725 (vector) / :747-775 (array: every slice along `dims` is a channel)
function resample(x::AbstractVector{T}, rate::Union{Integer,Rational}, h::Vector=resample_filter(rate)) where {T}
    S = fftintype(T)
    f = FIRFilter(convert(Vector{real(promote_type(eltype(h), S)) == Float32 ? Float32 : Float64}, h), rate; xtype=S)
    rate == 1 || setphase!(f, timedelay(f))                              # undelay!, :706-714
    outLen = ceil(Int, length(x) * rate)
    xp = zeros(S, inputlength(f, outLen, RoundUp)); xp[1:length(x)] .= x # _zeropad, :699
    y = filt(f, xp)
    length(y) >= outLen || throw(AssertionError("Resample output shorter than expected."))                  # :722
    y[1:outLen]
end
function resample(x::AbstractArray{T}, rate::Union{Integer,Rational}, h::Vector=resample_filter(rate); dims::Integer) where {T}
    S = fftintype(T)
    xm = reshape(permutedims(x, (dims, setdiff(1:ndims(x), dims)...)), size(x, dims), :)      # slices along `dims` as columns
    nch = size(xm, 2)
    f = FIRFilter(convert(Vector{real(promote_type(eltype(h), S)) == Float32 ? Float32 : Float64}, h), rate; xtype=S, nch)
    rate == 1 || setphase!(f, timedelay(f))
    outLen = ceil(Int, size(xm, 1) * rate)
    xp = zeros(S, inputlength(f, outLen, RoundUp), nch); xp[1:size(xm, 1), :] .= xm
    y = filt(f, xp)
    size(y, 1) >= outLen || throw(AssertionError("Resample output shorter than expected."))
    osz = (outLen, (size(x, d) for d in setdiff(1:ndims(x), dims))...)
    permutedims(reshape(y[1:outLen, :], osz), invperm((dims, setdiff(1:ndims(x), dims)...)))
end

# ------------------------------------------------------------------------------ FIRArbitrary (floating-point rate)
mutable struct FIRArbitraryFilter                                                        # stream_filt.jl:92-156
    h::Ptr{Cvoid}
    taps::Vector
    rate::Float64
    Nϕ::Int
    xtype::DataType
    nch::Int
end
function FIRFilter(taps::Vector{Th}, rate::AbstractFloat, Nϕ::Integer=32; xtype::DataType=Th, nch::Integer=1) where {Th<:Union{Float32,Float64}}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve taps check(ccall((:mdsp_firarb_create, lib), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Cdouble, Int64, Cint, Cint, Int64),
                                  p, pointer(taps), length(taps), Float64(rate), Nϕ, mdtype(Th), mdtype(xtype), nch))
    f = FIRArbitraryFilter(p[], taps, Float64(rate), Nϕ, xtype, nch)
    finalizer(x -> ccall((:mdsp_firarb_destroy, lib), Cint, (Ptr{Cvoid},), x.h), f)
    f
end
reset!(f::FIRArbitraryFilter) = (check(ccall((:mdsp_firarb_reset, lib), Cint, (Ptr{Cvoid},), f.h)); f)            # :260-276
setphase!(f::FIRArbitraryFilter, ϕ::Real) = check(ccall((:mdsp_firarb_setphase, lib), Cint, (Ptr{Cvoid}, Cdouble), f.h, ϕ))  # :231-239
function timedelay(f::FIRArbitraryFilter)                                                                          # :400-401
    τ = Ref{Cdouble}(0)
    check(ccall((:mdsp_firarb_timedelay, lib), Cint, (Ptr{Cvoid}, Ref{Cdouble}), f.h, τ)); τ[]
end
function firinfo(f::FIRArbitraryFilter)
    nϕ, tp, hl, od, Δ = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0)
    check(ccall((:mdsp_firarb_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}), f.h, nϕ, tp, hl, od, Δ))
    (Nϕ = Int(nϕ[]), tapsPerϕ = Int(tp[]), historyLen = Int(hl[]), outtype = JLTYPE[od[] + 1], Δ = Δ[])
end
# the reference's state (stream_filt.jl:96-104): ϕAccumulator, α, ϕIdx, inputDeficit, xIdx, history
function getstate(f::FIRArbitraryFilter)
    hl = firinfo(f).historyLen
    hist = zeros(f.xtype, max(hl, 1), f.nch)
    acc, α = Ref{Cdouble}(0), Ref{Cdouble}(0)
    ϕ, d, xi = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    GC.@preserve hist check(ccall((:mdsp_firarb_get_state, lib), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}),
                                  f.h, acc, α, ϕ, d, xi, pointer(hist)))
    (ϕAccumulator = acc[], α = α[], ϕIdx = Int(ϕ[]), inputDeficit = Int(d[]), xIdx = Int(xi[]), history = hist[1:hl, :])
end
function setstate!(f::FIRArbitraryFilter, ϕAccumulator::Real, inputDeficit::Integer, history::Union{Nothing,AbstractMatrix}=nothing)
    hist = history === nothing ? nothing : convert(Matrix{f.xtype}, history)
    GC.@preserve hist check(ccall((:mdsp_firarb_set_state, lib), Cint, (Ptr{Cvoid}, Cdouble, Int64, Ptr{Cvoid}), f.h, ϕAccumulator, inputDeficit,
                                  hist === nothing ? C_NULL : pointer(hist)))
    f
end
# trajectories evaluated by the device scan / by the serial host loop so far (diagnostics)
function scan_stats(f::FIRArbitraryFilter)
    a, b = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:mdsp_firarb_scan_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), f.h, a, b))
    (scanned = Int(a[]), serial = Int(b[]))
end
function outputlength(f::FIRArbitraryFilter, inlen::Integer)                                                       # :340-342
    o = Ref{Int64}(0)
    check(ccall((:mdsp_firarb_outputlength, lib), Cint, (Ptr{Cvoid}, Int64, Ref{Int64}), f.h, inlen, o)); Int(o[])
end
function inputlength(f::FIRArbitraryFilter, outlen::Integer, r::RoundingMode=RoundDown)                            # :385-389
    o = Ref{Int64}(0)
    check(ccall((:mdsp_firarb_inputlength, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Ref{Int64}), f.h, outlen,
                (r == RoundUp || r == RoundFromZero) ? 1 : 0, o)); Int(o[])
end
# filt(f, x): buffer of outputlength + 1 samples, resized to samplesWritten (allocate_output :639-655, filt :627-637)
function filt(f::FIRArbitraryFilter, x::Union{AbstractVecOrMat,DeviceArray})
    xd = todevice(x, f.xtype)
    xlen = size(xd, 1)
    ycap = max(outputlength(f, xlen), 0) + 1
    y = DeviceArray{firinfo(f).outtype}(f.nch == 1 ? (ycap,) : (ycap, f.nch))
    nw = Ref{Int64}(0)
    check(ccall((:mdsp_firarb_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ref{Int64}, Ptr{Cvoid}),
                f.h, xd.ptr, xlen, xlen, y.ptr, ycap, ycap, nw, C_NULL))
    yh = back(y, x)
    yh isa DeviceArray ? yh : (ndims(yh) == 1 ? yh[1:nw[]] : yh[1:nw[], :])
end
filt(h::Vector, x::AbstractVector, rate::AbstractFloat, Nϕ::Integer=32) = filt(FIRFilter(h, rate, Nϕ; xtype=fftintype(eltype(x))), x)   # :669-672
# resample(x, rate::AbstractFloat[, h, Nϕ = 32])   stream_filt.jl:692-694, :752-755
function resample(x::AbstractVecOrMat{T}, rate::AbstractFloat, h::Vector=resample_filter(rate), Nϕ::Integer=32) where {T}
    S = fftintype(T)
    nch = size(x, 2)
    f = FIRFilter(convert(Vector{real(promote_type(eltype(h), S)) == Float32 ? Float32 : Float64}, h), rate, Nϕ; xtype=S, nch)
    setphase!(f, timedelay(f))                                          # undelay!
    outLen = ceil(Int, size(x, 1) * rate)
    npad = inputlength(f, outLen, RoundUp)
    xp = zeros(S, npad, nch); xp[1:size(x, 1), :] .= x
    y = filt(f, ndims(x) == 1 ? vec(xp) : xp)
    size(y, 1) >= outLen || throw(AssertionError("Resample output shorter than expected."))   # :722
    ndims(x) == 1 ? y[1:outLen] : y[1:outLen, :]
end
# the serial phase-accumulator recurrence on the host and its parallel evaluation (tests compare the two bit for bit)
function arb_trajectory(ϕAcc::Real, inputDeficit::Integer, rate::Real, Nϕ::Integer, xlen::Integer, block::Integer, cap::Integer)
    ax, aa = zeros(Int64, cap), zeros(Float64, cap)
    nout, dend = Ref{Int64}(0), Ref{Int64}(0)
    aend = Ref{Cdouble}(0)
    GC.@preserve ax aa check(ccall((:mdsp_arb_trajectory, lib), Cint,
        (Cdouble, Int64, Cdouble, Int64, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64, Ref{Int64}, Ref{Cdouble}, Ref{Int64}),
        ϕAcc, inputDeficit, rate, Nϕ, xlen, block, pointer(ax), pointer(aa), cap, nout, aend, dend))
    (anchors_x = ax, anchors_acc = aa, nout = Int(nout[]), ϕAcc_end = aend[], deficit_end = Int(dend[]))
end

# the host emulation of the device's parallel evaluation of the same recurrence (used == false: the scan does not apply to these arguments)
function arb_trajectory_scan(ϕAcc::Real, inputDeficit::Integer, rate::Real, Nϕ::Integer, xlen::Integer, pilot::Integer, cap::Integer)
    ax, aa = zeros(Int64, cap), zeros(Float64, cap)
    nout, dend = Ref{Int64}(0), Ref{Int64}(0)
    aend = Ref{Cdouble}(0)
    used, passes = Ref{Cint}(0), Ref{Cint}(0)
    GC.@preserve ax aa check(ccall((:mdsp_arb_trajectory_scan, lib), Cint,
        (Cdouble, Int64, Cdouble, Int64, Int64, Int64, Ptr{Int64}, Ptr{Cdouble}, Int64, Ref{Int64}, Ref{Cdouble}, Ref{Int64}, Ref{Cint}, Ref{Cint}),
        ϕAcc, inputDeficit, rate, Nϕ, xlen, pilot, pointer(ax), pointer(aa), cap, nout, aend, dend, used, passes))
    (used = used[] != 0, passes = Int(passes[]), anchors_x = ax, anchors_acc = aa, nout = Int(nout[]), ϕAcc_end = aend[], deficit_end = Int(dend[]))
end
# updates at which the device replay's branch-free form of update! (stream_filt.jl:567-577) would differ from the reference form: always 0
function arb_replay_check(ϕAcc::Real, rate::Real, Nϕ::Integer, nsteps::Integer)
    m = Ref{Int64}(0)
    check(ccall((:mdsp_arb_replay_check, lib), Cint, (Cdouble, Cdouble, Int64, Int64, Ref{Int64}), ϕAcc, rate, Nϕ, nsteps, m)); Int(m[])
end
# the launch geometry of the arbitrary-rate kernel (the host function the launch itself calls; cu <= 0: the current device's compute units)
function arb_kernel_geometry(tapsPerϕ::Integer, Nϕ::Integer, rate::Real, ::Type{Th}, ::Type{Tx}, nch::Integer, nout::Integer, cu::Integer=0) where {Th,Tx}
    o = zeros(Int64, 8)
    GC.@preserve o check(ccall((:mdsp_arb_kernel_geometry, lib), Cint, (Int64, Int64, Cdouble, Cint, Cint, Int64, Int64, Cint, Ptr{Int64}),
                               tapsPerϕ, Nϕ, rate, mdtype(Th), mdtype(Tx), nch, nout, cu, pointer(o)))
    (tile = Int(o[1]), span = Int(o[2]), nchg = Int(o[3]), groups = Int(o[4]), tiles = Int(o[5]), gy = Int(o[6]), taps_in_lds = o[7] != 0, lds_bytes = Int(o[8]))
end

# ---------------------------------------------------------------------------------------------- DF2TFilter (FIR) and filtfilt
# DF2TFilter(PolynomialRatio(b, [1]))   Filters/filt.jl:122-181: the TDF-II register file `state` (length(b) - 1, columns) is carried between calls
mutable struct DF2TFilter{T}
    b::Vector{T}
    state::Matrix{T}
end
function DF2TFilter(b::AbstractVector{<:Real}, a::Union{Real,AbstractVector{<:Real}}=1.0; coldims::Integer=1)
    a1 = a isa Real ? a : (length(a) == 1 ? a[1] : throw(UnsupportedError("IIR DF2TFilter is a serial recursion; only FIR coefficients run on the device")))
    isempty(b) && throw(ArgumentError("filter coefficients must be non-empty"))
    a1 == 0 && throw(ArgumentError("filter vector a[1] must be nonzero"))
    T = eltype(b) == Float32 ? Float32 : Float64
    taps = convert(Vector{T}, a1 == 1 ? b : b ./ a1)                                    # PolynomialRatio normalises by a[1]
    DF2TFilter{T}(taps, zeros(T, length(taps) - 1, coldims))
end
function filt(f::DF2TFilter{T}, x::AbstractVecOrMat{Tx}) where {T,Tx<:Real}
    size(x, 2) == size(f.state, 2) || throw(ArgumentError("state size must match x"))   # :158
    W = promote_type(T, fftintype(Tx))
    nb = length(f.b)
    nb == 1 && return convert(Array{W}, x) .* f.b[1]                                    # mul!(out, x, b[1]), :163
    xd = todevice(x, W)
    nx = size(xd, 1)
    y = DeviceArray{W}(size(xd))
    si = upload(convert(Matrix{W}, f.state))
    taps = convert(Vector{W}, f.b)
    GC.@preserve taps (nx > 0 && check(ccall((:mdsp_tdfir_state_exec, lib), Cint,
        (Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        pointer(taps), nb, mdtype(W), xd.ptr, nx, ncolumns(xd), nx, y.ptr, nx, si.ptr, C_NULL)))
    f.state = convert(Matrix{T}, download(si))
    download(y)
end
# complex coefficients: the TDF-II state is complex (zeros(promote_type(T, V), ...), filt.jl:149-151) and the signal enters the recursion widened to it
function DF2TFilter(b::AbstractVector{<:Complex}, a::Number=1.0; coldims::Integer=1)
    isempty(b) && throw(ArgumentError("filter coefficients must be non-empty"))
    a == 0 && throw(ArgumentError("filter vector a[1] must be nonzero"))
    T = eltype(b) == ComplexF32 ? ComplexF32 : ComplexF64
    taps = convert(Vector{T}, a == 1 ? b : b ./ a)
    DF2TFilter{T}(taps, zeros(T, length(taps) - 1, coldims))
end
function filt(f::DF2TFilter{T}, x::AbstractVecOrMat{Tx}) where {T<:Complex,Tx<:Number}
    size(x, 2) == size(f.state, 2) || throw(ArgumentError("state size must match x"))
    W = promote_type(T, fftintype(Tx))
    nb = length(f.b)
    nb == 1 && return convert(Array{W}, x) .* f.b[1]
    xd = todevice(x, W)
    nx = size(xd, 1)
    y = DeviceArray{W}(size(xd))
    si = upload(convert(Matrix{W}, f.state))
    taps = convert(Vector{W}, f.b)
    GC.@preserve taps (nx > 0 && check(ccall((:mdsp_tdfir_state_exec_t, lib), Cint,
        (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        pointer(taps), nb, mdtype(W), mdtype(W), xd.ptr, nx, ncolumns(xd), nx, y.ptr, nx, si.ptr, C_NULL)))
    f.state = convert(Matrix{T}, download(si))
    download(y)
end
# filtfilt(b, x) / filtfilt(b, a, x) with scalar a   filt.jl:301-338: odd-symmetric extension, one pass with conv(b, reverse(b)), trim
function filtfilt(b::AbstractVector{<:Real}, x::AbstractVecOrMat{Tx}) where {Tx<:Real}
    nb, n = length(b), size(x, 1)
    nb - 1 <= n - 1 || throw(ArgumentError("the signal must be longer than the filter order"))
    bw = convert(Vector{eltype(b) == Float32 ? Float32 : Float64}, b)
    newb = conv(bw, reverse(bw); algorithm=:direct)                                     # :309-314
    W = promote_type(eltype(bw), fftintype(Tx))
    xd = todevice(x, W)
    ext = DeviceArray{W}(ndims(x) == 1 ? (n + 2 * (nb - 1),) : (n + 2 * (nb - 1), size(x, 2)))
    n > 0 && check(ccall((:mdsp_extrapolate, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                         xd.ptr, n, ncolumns(xd), n, mdtype(W), nb - 1, ext.ptr, n + 2 * (nb - 1), C_NULL))   # extrapolate_signal!, :243-257
    y = download(filt(newb, ext))                                                       # filt!(extrapolated, newb, extrapolated), :322
    ndims(x) == 1 ? y[2nb-1:end] : y[2nb-1:end, :]                                      # drop garbage at start, :325
end
filtfilt(b::AbstractVector{<:Real}, a::Union{Real,AbstractVector{<:Real}}, x) =
    (a isa Real || length(a) == 1) ? filtfilt(b ./ (a isa Real ? a : a[1]), x) :
    throw(UnsupportedError("IIR filtfilt is a serial recursion; only FIR coefficients run on the device"))

# ------------------------------------------------------------------------------------------------ multitaper
# dpss(n, nw, ntapers)   windows.jl:668-726: the Slepian tapers as eigenvectors of the symmetric tridiagonal matrix (host, like every window)
function dpss(n::Integer, nw::Real, ntapers::Integer=ceil(Int, 2 * nw) - 1)
    0 < ntapers <= n || throw(DomainError(ntapers, "ntapers must be in the interval (0, n]"))
    0 <= nw < n / 2 || throw(DomainError(nw, "nw must be in the interval [0, n/2)"))
    dv = [cospi(2 * nw / n) * ((n - 1) / 2 - i)^2 for i in 0:n-1]
    ev = [0.5 * (k * n - k^2) for k in 1:n-1]
    v = eigen(SymTridiagonal(dv, ev), n-ntapers+1:n).vectors[:, end:-1:1]
    for c in 1:ntapers       # sign conventions :696-707: symmetric tapers have a positive mean, skew ones a positive first lobe
        col = view(v, :, c)
        flip = isodd(c) ? sum(col) < 0 : col[findfirst(x -> abs(x) > 1e-12, col)] < 0
        flip && (col .*= -1)
    end
    v
end

# MTConfig{T}(n_samples; fs, nfft, window, nw, ntapers, taper_weights, onesided)   multitaper.jl:5-49, :112-135
mutable struct MTConfig{T}
    h::Ptr{Cvoid}
    n_samples::Int; fs::Float64; nfft::Int; ntapers::Int
    freq::AbstractVector; window::Matrix{Float64}; onesided::Bool; r::Vector{Float64}; nout::Int
end
function MTConfig{T}(n_samples::Integer; fs::Real=1, nfft::Integer=nextpow(2, n_samples), window::Union{Nothing,AbstractMatrix}=nothing, nw::Real=4,
                     ntapers::Integer=2 * nw - 1, taper_weights::AbstractVector=fill(1 / ntapers, ntapers), onesided::Bool=T <: Real,
                     engine=ENGINE_AUTO) where {T}
    onesided && T <: Complex && throw(ArgumentError("cannot compute one-sided FFT of a complex signal"))     # :115-117
    n_samples > 0 || throw(ArgumentError("`n_samples` must be positive"))                                   # :118
    nfft >= n_samples || throw(ArgumentError("Must have `nfft >= n_samples`"))                              # :119
    ntapers > 0 || throw(ArgumentError("`ntapers` must be positive"))                                       # :23
    fs > 0 || throw(ArgumentError("`fs` must be positive"))                                                 # :24
    if window === nothing
        r = fs ./ taper_weights                                                                              # :127
        window = dpss(n_samples, nw, ntapers)                                                                # :128
    else
        r = fs .* vec(sum(abs2, window; dims=1)) ./ taper_weights                                            # :130
    end
    size(window) == (n_samples, ntapers) || throw(DimensionMismatch("Must have `size(window) == (n_samples, ntapers)`"))   # :34-36
    size(r) == (ntapers,) || throw(DimensionMismatch("Must have `size(r) == (ntapers,)`"))                  # :37-39
    w = convert(Matrix{Float64}, window); rv = convert(Vector{Float64}, r)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve w rv check(ccall((:mdsp_mt_plan_create, lib), Cint, (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cint, Cint),
                                  p, n_samples, nfft, pointer(w), ntapers, pointer(rv), onesided, mdtype(fftintype(T)), engine))
    no, nt, eng = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0)
    check(ccall((:mdsp_mt_plan_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}), p[], no, nt, eng))
    c = MTConfig{T}(p[], n_samples, fs, nfft, ntapers, onesided ? rfftfreq(nfft, fs) : fftfreq(nfft, fs), w, onesided, rv, Int(no[]))
    finalizer(x -> ccall((:mdsp_mt_plan_destroy, lib), Cint, (Ptr{Cvoid},), x.h), c)
    c
end
# multitaper PSDs of the frames of every column of `signal`: (nout, K, nch) on the device   mt_pgram! :225-245, mt_spectrogram! :312-330
function mt_psd(config::MTConfig{T}, signal::AbstractVecOrMat, noverlap::Integer) where {T}
    sd = todevice(signal, fftintype(T))
    len = size(sd, 1); nch = ncolumns(sd)
    K = framecount(len, config.n_samples, noverlap)
    out = DeviceArray{fftabs2type(T)}((config.nout, K, nch))
    K > 0 && check(ccall((:mdsp_mt_psd_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                         config.h, sd.ptr, len, noverlap, nch, len, out.ptr, config.nout, K * config.nout, C_NULL))
    download(out)
end
# mt_pgram(s; ...) / mt_pgram(s, config) / mt_pgram!(output, s, config)   multitaper.jl:177-245
function mt_pgram(s::AbstractVector{T}, config::MTConfig) where {T}
    length(s) == config.n_samples || throw(DimensionMismatch("Expected `signal` to be of length `config.n_samples`; got `length(signal)` = $(length(s)) and `config.n_samples` = $(config.n_samples)"))
    Periodogram(mt_psd(config, s, 0)[:, 1, 1], config.freq)
end
mt_pgram(s::AbstractVector{T}; onesided::Bool=T <: Real, nfft::Int=nextfastfft(length(s)), fs::Real=1, nw::Real=4,
         ntapers::Int=ceil(Int, 2nw) - 1, window::Union{Nothing,AbstractMatrix}=nothing) where {T<:Number} =
    mt_pgram(s, MTConfig{fftintype(T)}(length(s); fs, nfft, window, nw, ntapers, onesided))
function mt_pgram!(output::AbstractVector, s::AbstractVector, config::MTConfig)
    length(output) == length(config.freq) || throw(DimensionMismatch("Expected `output` to be of length `length(config.freq)`; got `length(output)` = $(length(output)) and `length(config.freq)` = $(length(config.freq))"))
    copyto!(output, power(mt_pgram(s, config)))
    Periodogram(output, config.freq)
end
# MTSpectrogramConfig / mt_spectrogram / mt_spectrogram!   multitaper.jl:248-392
struct MTSpectrogramConfig{T}
    n_samples::Int
    n_overlap_samples::Int
    time::StepRangeLen{Float64,Base.TwicePrecision{Float64},Base.TwicePrecision{Float64}}
    mt_config::MTConfig{T}
end
function MTSpectrogramConfig(n_samples::Int, mt_config::MTConfig{T}, n_overlap_samples::Int) where {T}
    spw = mt_config.n_samples
    spw > n_overlap_samples || throw(ArgumentError("Need `samples_per_window > n_overlap_samples`; got `samples_per_window` = $spw and `n_overlap_samples` = $n_overlap_samples."))   # :264-266
    hop = spw - n_overlap_samples
    len = n_samples < spw ? 0 : div(n_samples - spw, hop) + 1
    MTSpectrogramConfig{T}(n_samples, n_overlap_samples, (spw / 2 : hop : (len - 1) * hop + spw / 2) / mt_config.fs, mt_config)   # :270
end
MTSpectrogramConfig{T}(n_samples::Int, samples_per_window::Int, n_overlap_samples::Int; fs::Real=1, kwargs...) where {T} =
    MTSpectrogramConfig(n_samples, MTConfig{T}(samples_per_window; fs, kwargs...), n_overlap_samples)
function mt_spectrogram(signal::AbstractVector, config::MTSpectrogramConfig)
    length(signal) == config.n_samples || throw(DimensionMismatch("Expected `signal` to be of length `config.n_samples`; got `length(signal)` = $(length(signal)) and `config.n_samples` = $(config.n_samples)"))
    Spectrogram(mt_psd(config.mt_config, signal, config.n_overlap_samples)[:, :, 1], config.mt_config.freq, config.time)
end
mt_spectrogram(signal::AbstractVector, mt_config::MTConfig, n_overlap::Int=mt_config.n_samples >> 1) =
    mt_spectrogram(signal, MTSpectrogramConfig(length(signal), mt_config, n_overlap))
mt_spectrogram(signal::AbstractVector{T}, n::Int=length(signal) >> 3, n_overlap::Int=n >> 1; fs::Real=1, onesided::Bool=T <: Real, kwargs...) where {T} =
    mt_spectrogram(signal, MTSpectrogramConfig{fftintype(T)}(length(signal), n, n_overlap; fs, onesided, kwargs...))
function mt_spectrogram!(destination::AbstractMatrix, signal::AbstractVector, config::MTSpectrogramConfig)
    size(destination) == (length(config.mt_config.freq), length(config.time)) ||
        throw(DimensionMismatch("Expected `destination` to be of size `(length(config.mt_config.freq), length(config.time))`"))   # :314-317
    copyto!(destination, power(mt_spectrogram(signal, config)))
    Spectrogram(destination, config.mt_config.freq, config.time)
end
# cross power spectra and coherence   multitaper.jl:409-817 (signal: n_channels x n_samples, like the reference)
struct CrossPowerSpectra{T,F,A<:AbstractArray{T,3}} <: TFR{T}
    power::A
    freq::F
end
struct Coherence{T,F,A<:AbstractArray{T,3}} <: TFR{T}
    coherence::A
    freq::F
end
coherence(c::Coherence) = c.coherence
struct MTCrossSpectraConfig{T}
    n_channels::Int
    mt_config::MTConfig{T}
    demean::Bool
    freq_inds::Vector{Int64}          # 1-based indices into mt_config.freq
    freq::AbstractVector
end
function MTCrossSpectraConfig(n_channels::Int, mt_config::MTConfig{T}; demean::Bool=false, freq_range=nothing) where {T}
    (T <: Real && mt_config.onesided) || throw(ArgumentError("Only real data is supported (with the default choice of `onesided=true`) for this operation."))   # :417-422
    inds = freq_range === nothing ? collect(Int64, 1:length(mt_config.freq)) :
           Int64[i for i in eachindex(mt_config.freq) if freq_range[1] < mt_config.freq[i] < freq_range[end]]   # :503
    MTCrossSpectraConfig{T}(n_channels, mt_config, demean, inds, mt_config.freq[inds])
end
MTCrossSpectraConfig{T}(n_channels::Int, n_samples::Int; fs::Real=1, demean::Bool=false, freq_range=nothing, kwargs...) where {T} =
    MTCrossSpectraConfig(n_channels, MTConfig{T}(n_samples; fs, kwargs...); demean, freq_range)
function cross_spectra_device(signal::AbstractMatrix, config::MTCrossSpectraConfig{T}) where {T}
    mc = config.mt_config
    size(signal) == (config.n_channels, mc.n_samples) ||
        throw(DimensionMismatch("Size of `signal` does not match `(config.n_channels, config.mt_config.n_samples)`; got `size(signal)`=$(size(signal))"))   # :557-560
    nch = config.n_channels
    sd = todevice(permutedims(signal), fftintype(T))                     # (n_samples, n_channels): one channel per column
    C = fftouttype(fftintype(T))
    xmt = DeviceArray{C}((mc.nout, mc.ntapers, nch))
    check(ccall((:mdsp_mt_spectra_exec, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                mc.h, sd.ptr, nch, mc.n_samples, config.demean, xmt.ptr, C_NULL))
    out = DeviceArray{C}((nch, nch, length(config.freq_inds)))
    fi = config.freq_inds .- 1
    GC.@preserve fi check(ccall((:mdsp_mt_cross_spectra, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                                mc.h, xmt.ptr, nch, pointer(fi), length(fi), out.ptr, C_NULL))
    out
end
mt_cross_power_spectra(signal::AbstractMatrix, config::MTCrossSpectraConfig) = CrossPowerSpectra(download(cross_spectra_device(signal, config)), config.freq)
mt_cross_power_spectra(signal::AbstractMatrix{T}; fs::Real=1, kwargs...) where {T} =
    mt_cross_power_spectra(signal, MTCrossSpectraConfig{fftintype(T)}(size(signal)...; fs, kwargs...))
function mt_cross_power_spectra!(output::AbstractArray{<:Any,3}, signal::AbstractMatrix, config::MTCrossSpectraConfig)
    size(output) == (config.n_channels, config.n_channels, length(config.freq_inds)) ||
        throw(DimensionMismatch("Size of `output` does not match `(config.n_channels, config.n_channels, length(config.freq_inds))`"))   # :561-564
    copyto!(output, power(mt_cross_power_spectra(signal, config)))
    CrossPowerSpectra(output, config.freq)
end
struct MTCoherenceConfig{T}
    cs_config::MTCrossSpectraConfig{T}
end
MTCoherenceConfig{T}(n_channels::Int, n_samples::Int; kwargs...) where {T} = MTCoherenceConfig{T}(MTCrossSpectraConfig{T}(n_channels, n_samples; kwargs...))
function mt_coherence(signal::AbstractMatrix, config::MTCoherenceConfig{T}) where {T}
    cs = cross_spectra_device(signal, config.cs_config)
    nch, nfi = size(cs, 1), size(cs, 3)
    R = fftabs2type(fftintype(T))
    out = DeviceArray{R}((nch, nch, nfi))
    check(ccall((:mdsp_coherence_from_cs, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}), cs.ptr, nch, nfi, mdtype(R), out.ptr, C_NULL))   # coherence_from_cs!, :704-723
    Coherence(download(out), config.cs_config.freq)
end
mt_coherence(signal::AbstractMatrix{T}; fs::Real=1, freq_range=nothing, demean::Bool=false, kwargs...) where {T} =
    mt_coherence(signal, MTCoherenceConfig{fftintype(T)}(size(signal)...; fs, freq_range, demean, kwargs...))
function mt_coherence!(output::AbstractArray{<:Any,3}, signal::AbstractMatrix, config::MTCoherenceConfig)
    size(output) == (config.cs_config.n_channels, config.cs_config.n_channels, length(config.cs_config.freq)) ||
        throw(DimensionMismatch("Size of `output` does not match `(config.cs_config.n_channels, config.cs_config.n_channels, length(config.cs_config.freq))`"))   # :774-777
    copyto!(output, coherence(mt_coherence(signal, config)))
    Coherence(output, config.cs_config.freq)
end

# ------------------------------------------------------------------------------------------------ yardsticks
# float4 copy / read / fill streams on the device (the bandwidth yardsticks bench.py quotes next to the kernels)
copy_bench!(dst::DeviceArray, src::DeviceArray) =
    check(ccall((:mdsp_copy_bench, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}), dst.ptr, src.ptr, length(src) * sizeof(eltype(src)), C_NULL))
copy_bench!(dst::DeviceArray, src::DeviceArray, mode::Integer, wgs_per_cu::Integer) =
    check(ccall((:mdsp_copy_bench_mode, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint, Cint, Ptr{Cvoid}), dst.ptr, src.ptr, length(src) * sizeof(eltype(src)), mode, wgs_per_cu, C_NULL))

end # module
