# HMMSpikeSorterHIP.jl -- drop-in overrides that route the hot path of HMMSpikeSorter.jl through
# libhmmsort_hip.so (include/hmmsort.h).
#
# NOT EXERCISED IN THE BUILD IMAGE: no Julia runtime is installed there.  The Python host
# (hmmspikesorter.jl_amd/api.py) binds the same entry points and is what the tests run.
#
# Usage:   using HMMSpikeSorter; include("HMMSpikeSorterHIP.jl"); HMMSpikeSorterHIP.enable!()
# After enable!(), HMMSpikeSorter.viterbi / forward / backward / update /
# train_model(X, sm, mu, sigma) / reconstruct_signal / fit(HMMSpikingModel, templates, X, chunksize) keep their
# signatures and return values (reference src/viterbi.jl:44, src/baumwelch.jl:25,73,205,362,
# src/reconstruction.jl:1, src/fit.jl:11) but run on the GPU.  Julia arrays are passed as they are: Matrix{Int16} states, Vector{Tuple{Int64,Int64,
# Float64}} transitions (24-byte isbits records), column-major Float64 matrices.
module HMMSpikeSorterHIP

using HMMSpikeSorter
import HMMSpikeSorter: StateMatrix, HMMSpikeTemplateModel, HMMSpikingModel

const lib = get(ENV, "HMMSORT_LIB", "libhmmsort_hip.so")

lasterror() = unsafe_string(ccall((:hmmsort_last_error, lib), Cstring, ()))
check(rc) = rc == 0 || error("hmmsort error $rc: $(lasterror())")

function viterbi(y::AbstractArray{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64)
    yv = y isa Array ? y : collect(y)          # fit.jl:23 passes contiguous views
    x = zeros(Int16, length(yv)); ll = Ref{Float64}(0.0)
    check(ccall((:hmmsort_viterbi, lib), Cint,
        (Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ptr{Int16}, Ref{Float64}),
        yv, length(yv), lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions), μ, σ, x, ll))
    x, ll[]
end

# the acquisition's Int16 samples (hmmsort.jl:79-88 converts them to Float64 on the host first): 2 bytes per
# sample cross PCIe and are widened in HBM; same decode as on the converted signal
function viterbi(y::AbstractArray{Int16,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64)
    yv = y isa Array ? y : collect(y)
    x = zeros(Int16, length(yv)); ll = Ref{Float64}(0.0)
    check(ccall((:hmmsort_viterbi_i16, lib), Cint,
        (Ptr{Int16}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ptr{Int16}, Ref{Float64}),
        yv, length(yv), lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions), μ, σ, x, ll))
    x, ll[]
end

# fit(HMMSpikingModel, templates, X, chunksize) (fit.jl:11-42, the CLI's call hmmsort.jl:90): the chunk loop, the
# stitch and the path stay on the device behind one call; the signal goes up once.  Where the reference dies on a
# chunk without a silent sample (BoundsError at fit.jl:26, endless loop at :41) this raises (HMMSORT_ENOSILENT).
function fit_chunked(templates::HMMSpikeTemplateModel, X::AbstractVector{T}, chunksize::Integer) where T <: Union{Float64,Int16}
    Xv = X isa Array ? X : collect(X)
    lA = templates.state_matrix
    ml_seq = zeros(Int16, length(Xv)); ll = Ref{Float64}(0.0)
    sym = T === Int16 ? :hmmsort_fit_chunked_i16 : :hmmsort_fit_chunked
    check(ccall((sym, lib), Cint,
        (Ptr{T}, Int64, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ptr{Int16}, Ref{Float64}),
        Xv, length(Xv), chunksize, lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions),
        templates.μ, templates.σ, ml_seq, ll))
    HMMSpikingModel(templates, ml_seq, ll[], X)
end

# sample types of hmmsort_fit_channels (include/hmmsort.h)
const HMMSORT_SAMPLES_I16 = Cint(0)
const HMMSORT_SAMPLES_F64 = Cint(3)

# struct hmmsort_model (include/hmmsort.h): the model arguments of viterbi, one record per channel
struct CModel
    states::Ptr{Int16}; N::Int64; K::Int64; S::Int64
    tr::Ptr{Cvoid}; R::Int64; mu::Ptr{Float64}; sigma::Float64
end

"""
    fit_channels(templates, X, chunksize; devices=Int[]) -> Vector{HMMSpikingModel}

The chunked decode of several recording channels in one call (`hmmsort_fit_channels`): `templates[c]` and `X[c]`
(all of one length, all `Float64` or all `Int16`) belong to channel `c`; `chunksize <= 0` decodes every channel
whole.  Channel `c` runs on `devices[c % length(devices) + 1]` (0-based device numbers; empty: the current
device), channels on one device in step on streams of their own (option "fit_streams").  An extension: the
reference sorts one channel per process (hmmsort.jl:79-90).
"""
function fit_channels(templates::Vector{HMMSpikeTemplateModel}, X::Vector{Vector{T}}, chunksize::Integer;
                      devices::Vector{<:Integer}=Int[]) where T <: Union{Float64,Int16}
    C = length(X); n = length(X[1])
    length(templates) == C && all(length(x) == n for x in X) || error("fit_channels: one model per channel, equal lengths")
    ml = [zeros(Int16, n) for _ in 1:C]; ll = zeros(Float64, C); status = zeros(Cint, C)
    dev = Cint.(devices)
    GC.@preserve templates X ml dev begin
        models = [CModel(pointer(t.state_matrix.states), t.state_matrix.N, t.state_matrix.K, t.state_matrix.nstates,
                         Ptr{Cvoid}(pointer(t.state_matrix.transitions)), length(t.state_matrix.transitions),
                         pointer(t.μ), t.σ) for t in templates]
        ys = [Ptr{Cvoid}(pointer(x)) for x in X]; outs = [pointer(m) for m in ml]
        check(ccall((:hmmsort_fit_channels, lib), Cint,
            (Int64, Ptr{Ptr{Cvoid}}, Cint, Int64, Int64, Ptr{CModel}, Ptr{Cint}, Int64, Ptr{Ptr{Int16}}, Ptr{Float64},
             Ptr{Cint}),
            C, ys, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, n, chunksize, models, isempty(dev) ? Ptr{Cint}(C_NULL) : pointer(dev),
            length(dev), outs, ll, status))
    end
    [HMMSpikingModel(templates[c], ml[c], ll[c], X[c]) for c in 1:C]
end

function _fb(sym, V, lA, μ, σ)
    a = Array{Float64,2}(undef, lA.nstates, length(V))
    check(ccall((sym, lib), Cint,
        (Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Float64}),
        V, length(V), lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions), μ, σ, a))
    a
end
forward(V::Array{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = _fb(:hmmsort_forward, V, lA, μ, σ)
backward(V::Array{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = _fb(:hmmsort_backward, V, lA, μ, σ)

function _finish(lA, μ, σnew, lp, nlp, pp)
    # baumwelch.jl:265 -- the rebuilt StateMatrix is a genuine reference struct
    lA_new = StateMatrix(lA.states .- one(Int16), pp, lA.K, lp[1:nlp[]]; allow_overlaps=lA.resolve_overlaps)
    lA_new, μ, σnew[]
end

function update(α::Array{Float64,2}, β::Array{Float64,2}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64, x::Array{Float64,1})
    σnew = Ref{Float64}(0.0); nlp = Ref{Int64}(0)
    lp = zeros(length(lA.transitions)); pp = zeros(lA.nstates)
    check(ccall((:hmmsort_update, lib), Cint,
        (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64,
         Ptr{Float64}, Float64, Ref{Float64}, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
        α, β, x, length(x), lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions),
        μ, σ, σnew, lp, length(lp), nlp, pp))       # μ is overwritten in place (baumwelch.jl:268)
    _finish(lA, μ, σnew, lp, nlp, pp)
end

# one EM step, baumwelch.jl:362-370: a single call, alpha/beta never leave the GPU.  The library keeps the
# plan (workspace, signal buffer) of the previous call of the same shape and re-arms it, so the EM loop of
# baumwelch.jl:324-354 pays the PCIe copy of X and the sweeps per step, not a plan build (2.7 ms per step at
# 10 M samples; `shutdown()` frees the cache).  Host threads may call concurrently.
function train_model(X::Array{Float64,1}, state_matrix::StateMatrix, μ0::Array{Float64,2}, σ0::Float64; verbose=0)
    σnew = Ref{Float64}(0.0); nlp = Ref{Int64}(0)
    lp = zeros(length(state_matrix.transitions)); pp = zeros(state_matrix.nstates)
    check(ccall((:hmmsort_em_step, lib), Cint,
        (Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ref{Float64}, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}),
        X, length(X), state_matrix.states, state_matrix.N, state_matrix.K, state_matrix.nstates,
        state_matrix.transitions, length(state_matrix.transitions), μ0, σ0, σnew, lp, length(lp), nlp, pp))
    _finish(state_matrix, μ0, σnew, lp, nlp, pp)
end

"""
    viterbi_step(X, state_matrix, μ0, σ0; return_path=false) -> (state_matrix′, μ′, σ′[, x, ll])

One step of Viterbi training (hard EM; an extension, INTEGRATION.md "Viterbi training"): decode `X`, then
re-estimate the model from the decoded path -- `update` with γ and ξ the indicators of that path.  One call;
signal and path stay on the GPU between the two halves.  `μ0` is overwritten in place like `train_model`'s.
It refines a model (templates from a spike sorter, or after Baum-Welch); from a random start the decode holds no
spike and every template would lose its entry transition.
"""
function viterbi_step(X::Array{Float64,1}, state_matrix::StateMatrix, μ0::Array{Float64,2}, σ0::Float64; return_path=false)
    σnew = Ref{Float64}(0.0); nlp = Ref{Int64}(0); ll = Ref{Float64}(0.0)
    lp = zeros(length(state_matrix.transitions)); pp = zeros(state_matrix.nstates)
    x = zeros(Int16, return_path ? length(X) : 0)
    check(ccall((:hmmsort_viterbi_step, lib), Cint,
        (Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ref{Float64}, Ptr{Float64}, Int64, Ref{Int64}, Ptr{Float64}, Ptr{Int16}, Ref{Float64}),
        X, length(X), state_matrix.states, state_matrix.N, state_matrix.K, state_matrix.nstates,
        state_matrix.transitions, length(state_matrix.transitions), μ0, σ0, σnew, lp, length(lp), nlp, pp,
        return_path ? pointer(x) : Ptr{Int16}(C_NULL), ll))
    out = _finish(state_matrix, μ0, σnew, lp, nlp, pp)
    return_path ? (out..., x, ll[]) : out
end

# struct hmmsort_step_out (include/hmmsort.h): what hmmsort_fit_step_channels returns per channel
struct CStepOut
    mu::Ptr{Float64}; sigma::Ptr{Float64}; lp::Ptr{Float64}; lp_cap::Int64; n_lp::Ptr{Int64}
    pp::Ptr{Float64}; counts::Ptr{Int64}
end

"""
    fit_step_channels(templates, X, chunksize; devices=Int[], pooled=false) -> (models, steps)

One step of Viterbi training for several channels in one call (`hmmsort_fit_step_channels`, INTEGRATION.md
"Viterbi training"): every channel is decoded as `fit_channels` decodes it, and re-estimated from the statistics of
its stitched path while signal and path are on the GPU.  `steps[c] = (state_matrix′, μ′, σ′)`; with `pooled` the
channels' statistics are added in channel order and finished with the first channel's model: `steps` has one entry
(its first column is the old model's).
"""
function fit_step_channels(templates::Vector{HMMSpikeTemplateModel}, X::Vector{Vector{T}}, chunksize::Integer;
                           devices::Vector{<:Integer}=Int[], pooled::Bool=false) where T <: Union{Float64,Int16}
    C = length(X); n = length(X[1]); nout = pooled ? 1 : C
    length(templates) == C && all(length(x) == n for x in X) || error("fit_step_channels: one model per channel, equal lengths")
    ml = [zeros(Int16, n) for _ in 1:C]; ll = zeros(Float64, C); status = zeros(Cint, C)
    dev = Cint.(devices)
    sms = [t.state_matrix for t in templates[1:nout]]
    μs = [zeros(Float64, s.K, s.N) for s in sms]; σs = [zeros(Float64, 1) for _ in sms]
    lps = [zeros(Float64, length(s.transitions)) for s in sms]; nlps = [zeros(Int64, 1) for _ in sms]
    pps = [zeros(Float64, s.nstates) for s in sms]
    GC.@preserve templates X ml dev μs σs lps nlps pps begin
        models = [CModel(pointer(t.state_matrix.states), t.state_matrix.N, t.state_matrix.K, t.state_matrix.nstates,
                         Ptr{Cvoid}(pointer(t.state_matrix.transitions)), length(t.state_matrix.transitions),
                         pointer(t.μ), t.σ) for t in templates]
        recs = [CStepOut(pointer(μs[c]), pointer(σs[c]), pointer(lps[c]), length(lps[c]), pointer(nlps[c]),
                         pooled ? Ptr{Float64}(C_NULL) : pointer(pps[c]), Ptr{Int64}(C_NULL)) for c in 1:nout]
        ys = [Ptr{Cvoid}(pointer(x)) for x in X]; outs = [pointer(m) for m in ml]
        check(ccall((:hmmsort_fit_step_channels, lib), Cint,
            (Int64, Ptr{Ptr{Cvoid}}, Cint, Int64, Int64, Ptr{CModel}, Ptr{Cint}, Int64, Cint, Ptr{Ptr{Int16}},
             Ptr{Float64}, Ptr{CStepOut}, Ptr{Cint}),
            C, ys, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, n, chunksize, models,
            isempty(dev) ? Ptr{Cint}(C_NULL) : pointer(dev), length(dev), pooled ? 1 : 0, outs, ll, recs, status))
    end
    steps = [_finish(sms[c], μs[c], Ref(σs[c][1]), lps[c], Ref(nlps[c][1]), pooled ? sms[c].π : pps[c]) for c in 1:nout]
    [HMMSpikingModel(templates[c], ml[c], ll[c], X[c]) for c in 1:C], steps
end

# The additive statistics of Viterbi training on the device-resident plan API (include/hmmsort.h): `plan` is a
# hmmsort_plan*, the arrays are device pointers, `stream` a hipStream_t or C_NULL.  T is the length of the arrays.
path_stats_len(plan::Ptr{Cvoid}) = ccall((:hmmsort_plan_path_stats_len, lib), Int64, (Ptr{Cvoid},), plan)
path_stats!(plan::Ptr{Cvoid}, d_y::Ptr{Float64}, d_x::Ptr{Int16}, T::Integer, own_lo::Integer, own_hi::Integer,
            first::Bool, d_stats::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:hmmsort_plan_path_stats, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int16}, Int64, Int64, Int64, Cint, Ptr{Float64}, Ptr{Cvoid}),
        plan, d_y, d_x, T, own_lo, own_hi, first ? 1 : 0, d_stats, stream))
path_finish!(plan::Ptr{Cvoid}, d_stats::Ptr{Float64}, d_out::Ptr{Float64}, d_counts::Ptr{Int64}=Ptr{Int64}(C_NULL),
             stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:hmmsort_plan_path_finish, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}), plan, d_stats, d_out, d_counts, stream))
stats_sum!(d_parts::Ptr{Float64}, nparts::Integer, len::Integer, d_out::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:hmmsort_stats_sum, lib), Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}),
        d_parts, nparts, len, d_out, stream))

stats_blend!(d_acc::Ptr{Float64}, w::Float64, d_new::Ptr{Float64}, len::Integer, plain_tail::Integer=3,
             stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:hmmsort_stats_blend, lib), Cint, (Ptr{Float64}, Float64, Ptr{Float64}, Int64, Int64, Ptr{Cvoid}),
        d_acc, w, d_new, len, plain_tail, stream))

# struct hmmsort_adapt / hmmsort_track (include/hmmsort.h)
struct CAdapt
    halflife::Float64; warmup::Int64; update_sigma::Cint; update_lp::Cint
end
struct CTrack
    cap::Int64; n::Ptr{Int64}; first::Ptr{Int64}; own::Ptr{Int64}; w::Ptr{Float64}; mu::Ptr{Float64}; sigma::Ptr{Float64}
end

"""
    fit_adaptive(templates, X, chunksize, halflife; warmup=0, update_sigma=true, update_lp=false, cap=...)
        -> (model, track, final)

The chunked decode with the model re-estimated between chunks (`hmmsort_fit_adaptive`; an extension, INTEGRATION.md
"Drift tracking"): templates follow slow changes of the recording.  `track` = (n, first, own, w, μ, σ) with one entry
per chunk (`μ[:, :, c]` is what chunk `c` was decoded with); `final` = (state_matrix′, μ′, σ′), the full re-estimate
after the last chunk.  `cap` records are kept (default: twice the chunks of an even split, plus two).
"""
function fit_adaptive(templates::HMMSpikeTemplateModel, X::Vector{T}, chunksize::Integer, halflife::Real;
                      warmup::Integer=0, update_sigma::Bool=true, update_lp::Bool=false,
                      cap::Integer=chunksize > 0 ? 2 * (length(X) ÷ chunksize + 1) + 2 : 1) where T <: Union{Float64,Int16}
    sm = templates.state_matrix; n = length(X)
    ml = zeros(Int16, n); ll = Ref{Float64}(0.0)
    nrec = zeros(Int64, 1); first = zeros(Int64, cap); own = zeros(Int64, 2, cap); w = zeros(Float64, cap)
    μt = zeros(Float64, sm.K, sm.N, cap); σt = zeros(Float64, cap)
    μf = zeros(Float64, sm.K, sm.N); σf = zeros(Float64, 1); lpf = zeros(Float64, length(sm.transitions))
    nlpf = zeros(Int64, 1); ppf = zeros(Float64, sm.nstates)
    GC.@preserve templates X ml nrec first own w μt σt μf σf lpf nlpf ppf begin
        model = Ref(CModel(pointer(sm.states), sm.N, sm.K, sm.nstates, Ptr{Cvoid}(pointer(sm.transitions)),
                           length(sm.transitions), pointer(templates.μ), templates.σ))
        opt = Ref(CAdapt(Float64(halflife), warmup, update_sigma ? 1 : 0, update_lp ? 1 : 0))
        track = Ref(CTrack(cap, pointer(nrec), pointer(first), pointer(own), pointer(w), pointer(μt), pointer(σt)))
        fin = Ref(CStepOut(pointer(μf), pointer(σf), pointer(lpf), length(lpf), pointer(nlpf), pointer(ppf),
                           Ptr{Int64}(C_NULL)))
        check(ccall((:hmmsort_fit_adaptive, lib), Cint,
            (Ptr{Cvoid}, Cint, Int64, Int64, Ref{CModel}, Ref{CAdapt}, Ptr{Int16}, Ref{Float64}, Ref{CTrack}, Ref{CStepOut}),
            X, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, n, chunksize, model, opt, ml, ll, track, fin))
    end
    m = min(nrec[1], cap)
    HMMSpikingModel(templates, ml, ll[], X),
        (n=nrec[1], first=first[1:m], own=own[:, 1:m], w=w[1:m], μ=μt[:, :, 1:m], σ=σt[1:m]),
        _finish(sm, μf, Ref(σf[1]), lpf, Ref(nlpf[1]), ppf)
end

"reconstruct_signal under the model track of `fit_adaptive` (`hmmsort_reconstruct_tracked`): sample t takes the templates of the last chunk that starts at or before it"
function reconstruct_tracked(x::Array{Int16,1}, lA::StateMatrix, first::Vector{Int64}, μtrack::Array{Float64,3})
    Y2 = zeros(Float64, length(x))
    check(ccall((:hmmsort_reconstruct_tracked, lib), Cint,
        (Ptr{Int16}, Int64, Ptr{Int16}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        x, length(x), lA.states, lA.N, lA.nstates, lA.K, length(first), first, μtrack, Y2))
    Y2
end

# struct hmmsort_seed_opt / hmmsort_seed_out (include/hmmsort.h)
struct CSeedOpt
    threshold::Float64; sigma::Float64; polarity::Cint; align::Int64; refractory::Int64; max_iters::Int64
end
struct CSeedOut
    mu::Ptr{Float64}; sigma::Ptr{Float64}; lp::Ptr{Float64}; counts::Ptr{Int64}; n_events::Ptr{Int64}
    iters::Ptr{Int64}; times::Ptr{Int64}; labels::Ptr{Int16}; cap::Int64
end

function _seed_finish(N, K, resolve_overlaps, μ, σ, lp, counts, ne, iters, times, labels)
    E = ne[1]; kept = findall(counts .> 0)
    info = (counts=counts[kept], times=times[1:E], labels=labels[1:E] .+ Int16(1), iters=iters[1], kept=kept)
    isempty(kept) && return StateMatrix(), zeros(Float64, K, 0), σ[1], info
    StateMatrix(length(kept), K, lp[kept], resolve_overlaps), μ[:, kept], σ[1], info
end

"""
    seed_templates(X, N=3, K=60, resolve_overlaps=false; threshold=NaN, sigma=0.0, polarity=0, align=-1,
                   refractory=-1, max_iters=0) -> (state_matrix, μ, σ, info)

Templates from the recording alone (`hmmsort_seed_templates`; an extension with no counterpart in the reference, which
starts `train_model` from random templates and takes sorting templates from a file; INTEGRATION.md "Template seed"):
threshold crossings that are the extremum of their ±refractory window, clustered into `N` groups on the device.  The
keyword defaults ask for the library's (4.0 noise scales, the robust noise estimate, |X|, (K-1)÷3, K-1, 20).  Empty
clusters are dropped; `info.labels` are 1-based cluster numbers before that, `info.kept` the clusters that survived.
`seed_templates_device` takes a resident signal.
"""
function seed_templates(X::Vector{T}, N::Integer=3, K::Integer=60, resolve_overlaps::Bool=false; threshold=NaN,
                        sigma=0.0, polarity=0, align=-1, refractory=-1, max_iters=0) where T <: Union{Float64,Int16}
    n = length(X); cap = n ÷ ((refractory >= 0 ? refractory : K - 1) + 1) + 1
    μ = zeros(Float64, K, N); σ = zeros(Float64, 1); lp = zeros(Float64, N); counts = zeros(Int64, N)
    ne = zeros(Int64, 1); iters = zeros(Int64, 1); times = zeros(Int64, cap); labels = zeros(Int16, cap)
    GC.@preserve X μ σ lp counts ne iters times labels begin
        opt = Ref(CSeedOpt(threshold, sigma, polarity, align, refractory, max_iters))
        out = Ref(CSeedOut(pointer(μ), pointer(σ), pointer(lp), pointer(counts), pointer(ne), pointer(iters),
                           pointer(times), pointer(labels), cap))
        check(ccall((:hmmsort_seed_templates, lib), Cint,
            (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ref{CSeedOpt}, Ref{CSeedOut}),
            X, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, n, N, K, opt, out))
    end
    _seed_finish(N, K, resolve_overlaps, μ, σ, lp, counts, ne, iters, times, labels)
end

"`seed_templates` of a float64 signal of `n` samples in device memory (`hmmsort_seed_templates_device`); synchronises `stream`"
function seed_templates_device(d_y::Ptr{Float64}, n::Integer, N::Integer=3, K::Integer=60,
                               resolve_overlaps::Bool=false; stream::Ptr{Cvoid}=C_NULL, threshold=NaN, sigma=0.0,
                               polarity=0, align=-1, refractory=-1, max_iters=0)
    cap = n ÷ ((refractory >= 0 ? refractory : K - 1) + 1) + 1
    μ = zeros(Float64, K, N); σ = zeros(Float64, 1); lp = zeros(Float64, N); counts = zeros(Int64, N)
    ne = zeros(Int64, 1); iters = zeros(Int64, 1); times = zeros(Int64, cap); labels = zeros(Int16, cap)
    GC.@preserve μ σ lp counts ne iters times labels begin
        opt = Ref(CSeedOpt(threshold, sigma, polarity, align, refractory, max_iters))
        out = Ref(CSeedOut(pointer(μ), pointer(σ), pointer(lp), pointer(counts), pointer(ne), pointer(iters),
                           pointer(times), pointer(labels), cap))
        check(ccall((:hmmsort_seed_templates_device, lib), Cint,
            (Ptr{Float64}, Int64, Int64, Int64, Ref{CSeedOpt}, Ref{CSeedOut}, Ptr{Cvoid}), d_y, n, N, K, opt, out, stream))
    end
    _seed_finish(N, K, resolve_overlaps, μ, σ, lp, counts, ne, iters, times, labels)
end

# struct hmmsort_pre_opt (include/hmmsort.h) and the constants of hmmsort_preprocess
struct CPreOpt
    taps::Ptr{Float64}; half::Int64; reference::Cint; group::Ptr{Int32}; keep::Ptr{Int32}; nkeep::Int64
end
const HMMSORT_SAMPLES_I32 = Cint(1)
const HMMSORT_SAMPLES_F32 = Cint(2)
const HMMSORT_LAYOUT_CHANNEL_MAJOR = Cint(0)
const HMMSORT_LAYOUT_SAMPLE_MAJOR = Cint(1)
const HMMSORT_REF = Dict(:none => Cint(0), :median => Cint(1), :mean => Cint(2))
_sample_type(::Type{Int16}) = HMMSORT_SAMPLES_I16
_sample_type(::Type{Int32}) = HMMSORT_SAMPLES_I32
_sample_type(::Type{Float32}) = HMMSORT_SAMPLES_F32
_sample_type(::Type{Float64}) = HMMSORT_SAMPLES_F64

# half of an odd-length symmetric filter, centre first; an empty vector stands for "no filter"
_half(taps::Vector{Float64}) = isempty(taps) ? Float64[] :
    (isodd(length(taps)) ? taps[(length(taps) + 1) ÷ 2:end] : error("preprocess: taps must have odd length"))

"""
    preprocess(raw; taps=Float64[], reference=:none, groups=Int32[], keep=Int32[], sample_major=false) -> Matrix{Float64}

Front end for a raw recording block (`hmmsort_preprocess`; an extension, INTEGRATION.md "Front end"; the reference reads a
channel an upstream tool has filtered, hmmsort.jl:66-88): a zero-phase FIR filter per channel (`taps`: the full
odd-length symmetric filter; empty: none), then the `:median` or `:mean` of every group of channels (`groups`: one id per
channel, negative: filtered only; empty: one group) subtracted per sample.  `raw` is the reference's `data` array,
samples × channels (column-major, so channel-major in memory), or channels × samples with `sample_major=true`, of
Int16, Int32, Float32 or Float64 samples; it goes to the device as it is.  `keep`: 1-based channels to return (empty:
all).  Returns samples × channels (one column per kept channel), Float64.
"""
function preprocess(raw::Matrix{T}; taps::Vector{Float64}=Float64[], reference::Symbol=:none,
                    groups::Vector{Int32}=Int32[], keep::Vector{<:Integer}=Int32[],
                    sample_major::Bool=false) where T <: Union{Int16,Int32,Float32,Float64}
    n, C = sample_major ? reverse(size(raw)) : size(raw)
    isempty(groups) || length(groups) == C || error("preprocess: groups needs one entry per channel")
    half = _half(taps); keep0 = Int32.(keep .- 1)
    out = zeros(Float64, n, isempty(keep0) ? C : length(keep0))
    GC.@preserve raw half groups keep0 out begin
        opt = Ref(CPreOpt(isempty(half) ? C_NULL : pointer(half), max(length(half) - 1, 0), HMMSORT_REF[reference],
                          isempty(groups) ? C_NULL : pointer(groups), isempty(keep0) ? C_NULL : pointer(keep0),
                          length(keep0)))
        check(ccall((:hmmsort_preprocess, lib), Cint,
            (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ref{CPreOpt}, Ptr{Float64}),
            raw, _sample_type(T), sample_major ? HMMSORT_LAYOUT_SAMPLE_MAJOR : HMMSORT_LAYOUT_CHANNEL_MAJOR, C, n, opt,
            out))
    end
    out
end

"`preprocess` of a block of `C` channels × `n` samples in device memory into the resident `[C][n]` Float64 array `d_out` the batched plans take (`hmmsort_preprocess_device`); `taps`, `groups` are host arrays; synchronises `stream`"
function preprocess_device(d_raw::Ptr{T}, layout::Cint, C::Integer, n::Integer, d_out::Ptr{Float64};
                           taps::Vector{Float64}=Float64[], reference::Symbol=:none, groups::Vector{Int32}=Int32[],
                           stream::Ptr{Cvoid}=C_NULL) where T <: Union{Int16,Int32,Float32,Float64}
    half = _half(taps)
    GC.@preserve half groups begin
        opt = Ref(CPreOpt(isempty(half) ? C_NULL : pointer(half), max(length(half) - 1, 0), HMMSORT_REF[reference],
                          isempty(groups) ? C_NULL : pointer(groups), C_NULL, 0))
        check(ccall((:hmmsort_preprocess_device, lib), Cint,
            (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ref{CPreOpt}, Ptr{Float64}, Ptr{Cvoid}),
            d_raw, _sample_type(T), layout, C, n, opt, d_out, stream))
    end
    d_out
end

# struct hmmsort_noise_opt / hmmsort_noise_out (include/hmmsort.h, "Spatial whitening")
struct CNoiseOpt
    threshold::Float64; thr::Ptr{Float64}; guard::Int64
end
struct CNoiseOut
    sigma::Ptr{Float64}; n_quiet::Ptr{Int64}; s1::Ptr{Float64}; s2::Ptr{Float64}; d_quiet::Ptr{UInt8}
end

"""
    noise_cov_device(d_y, C, n; threshold=4.0, guard=30, thr=Float64[], d_quiet=C_NULL, stream=C_NULL)
        -> (sigma, n_quiet, s1, s2)

Noise scale per channel, quiet mask and the raw sums over the quiet samples of the resident Float64 block `[C][n]`
(`hmmsort_noise_cov_device`; an extension, INTEGRATION.md "Front end").  `thr`: absolute thresholds per channel
(then `sigma` comes back empty); `d_quiet`: optional device array of `n` bytes that receives the mask.  The covariance
is `s2 / n_quiet - m m'` with `m = s1 / n_quiet`.  Synchronises `stream`.
"""
function noise_cov_device(d_y::Ptr{Float64}, C::Integer, n::Integer; threshold::Float64=4.0, guard::Integer=30,
                          thr::Vector{Float64}=Float64[], d_quiet::Ptr{UInt8}=Ptr{UInt8}(C_NULL),
                          stream::Ptr{Cvoid}=C_NULL)
    isempty(thr) || length(thr) == C || error("noise_cov_device: thr needs one entry per channel")
    sigma = zeros(Float64, C); nq = zeros(Int64, 1); s1 = zeros(Float64, C); s2 = zeros(Float64, C, C)
    GC.@preserve thr sigma nq s1 s2 begin
        opt = Ref(CNoiseOpt(threshold, isempty(thr) ? C_NULL : pointer(thr), guard))
        out = Ref(CNoiseOut(pointer(sigma), pointer(nq), pointer(s1), pointer(s2), d_quiet))
        check(ccall((:hmmsort_noise_cov_device, lib), Cint,
            (Ptr{Float64}, Int64, Int64, Ref{CNoiseOpt}, Ref{CNoiseOut}, Ptr{Cvoid}), d_y, C, n, opt, out, stream))
    end
    (isempty(thr) ? sigma : Float64[], nq[1], s1, s2)
end

"""
    channel_mix_device(d_in, C, n, nbr, w, d_out; stream=C_NULL) -> d_out

`out[r][t] = sum over m of w[r, m] * in[nbr[r, m]][t]` on the resident Float64 block `[C][n]`
(`hmmsort_channel_mix_device`): `nbr` (R × M, 1-based channels, 0 for an empty slot) and `w` (R × M) are host
matrices.  `d_out == d_in` mixes in place (R == C).  Synchronises `stream`.
"""
function channel_mix_device(d_in::Ptr{Float64}, C::Integer, n::Integer, nbr::Matrix{<:Integer}, w::Matrix{Float64},
                            d_out::Ptr{Float64}; stream::Ptr{Cvoid}=C_NULL)
    size(nbr) == size(w) || error("channel_mix_device: nbr and w must have the same size")
    R, M = size(nbr)
    nbr0 = Matrix{Int32}(permutedims(nbr .- 1)); wt = Matrix{Float64}(permutedims(w))    # row-major [R][M], 0-based
    GC.@preserve nbr0 wt begin
        check(ccall((:hmmsort_channel_mix_device, lib), Cint,
            (Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
            d_in, C, n, R, M, nbr0, wt, d_out, stream))
    end
    d_out
end

# struct hmmsort_spike_fit_out (include/hmmsort.h)
struct CSpikeFitOut
    times::Ptr{Int64}; amp::Ptr{Float64}; rss::Ptr{Float64}; energy::Ptr{Float64}; nused::Ptr{Int32}; cap::Int64
    counts::Ptr{Int64}; summary::Ptr{Float64}
end

# call(out::Ref{CSpikeFitOut}) -> code, repeated with a larger cap until every event fits
function _spike_fit_run(call, N, K, cap)
    while true
        times = zeros(Int64, cap, N); amp = zeros(Float64, cap, N); rss = zeros(Float64, cap, N)
        energy = zeros(Float64, cap, N); nused = zeros(Int32, cap, N); counts = zeros(Int64, N)
        summary = zeros(Float64, 8 + 3 * (K - 1), N)
        GC.@preserve times amp rss energy nused counts summary begin
            check(call(Ref(CSpikeFitOut(pointer(times), pointer(amp), pointer(rss), pointer(energy), pointer(nused), cap,
                                        pointer(counts), pointer(summary)))))
        end
        if maximum(counts) <= cap
            return [(times=times[1:counts[a], a], amp=amp[1:counts[a], a], rss=rss[1:counts[a], a],
                     energy=energy[1:counts[a], a], nused=nused[1:counts[a], a], summary=summary[:, a]) for a in 1:N]
        end
        cap = maximum(counts)
    end
end

"""
    spike_fit(y, x, lA, μ[, first, μtrack]) -> one (times, amp, rss, energy, nused, summary) per template

Per-spike amplitude and residual of the path `x` of `y` (`hmmsort_spike_fit`; an extension, INTEGRATION.md "Spike fit"):
for every spike `extract_spiketimes` reports, the least-squares amplitude of its template on the samples under it once
the other templates the path says are active are taken out, the residual at unit amplitude and the window's energy;
`summary` holds the per-template sums (include/hmmsort.h).  `first`, `μtrack`: the model track of `fit_adaptive`.
`spike_fit_device` takes a plan and resident buffers of the plan's length.
"""
function spike_fit(y::Vector{T}, x::Vector{Int16}, lA::StateMatrix, μ::Array{Float64,2},
                   first::Vector{Int64}=Int64[], μtrack::Array{Float64,3}=zeros(Float64, 0, 0, 0)) where T <: Union{Float64,Int16}
    K = size(μ, 1)
    GC.@preserve y x μ first μtrack begin
        _spike_fit_run(lA.N, K, max(1, length(x) ÷ 8)) do out
            ccall((:hmmsort_spike_fit, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int16}, Ptr{Int16}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64},
                 Ptr{Float64}, Ref{CSpikeFitOut}),
                y, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, length(y), x, lA.states, lA.N, lA.nstates, μ, K,
                length(first), first, μtrack, out)
        end
    end
end

"`spike_fit` of a signal and path in device memory under the plan's current model (`hmmsort_plan_spike_fit`); synchronises `stream`"
function spike_fit_device(plan::Ptr{Cvoid}, d_y::Ptr{Float64}, d_x::Ptr{Int16}, n::Integer, N::Integer, K::Integer,
                          first::Vector{Int64}=Int64[], μtrack::Array{Float64,3}=zeros(Float64, 0, 0, 0);
                          stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve first μtrack begin
        _spike_fit_run(N, K, max(1, n ÷ 8)) do out
            ccall((:hmmsort_plan_spike_fit, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int16}, Int64, Ptr{Int64}, Ptr{Float64}, Ref{CSpikeFitOut}, Ptr{Cvoid}),
                plan, d_y, d_x, length(first), first, μtrack, out, stream)
        end
    end
end

# struct hmmsort_fp_opt / hmmsort_fp_out (include/hmmsort.h)
struct CFpOpt
    pre::Int64; W::Int64; M::Int64; chan::Ptr{Int32}
end
struct CFpOut
    sum::Ptr{Float64}; sumsq::Ptr{Float64}; nused::Ptr{Int64}; n::Ptr{Int64}
end

# call(opt::Ref{CFpOpt}, out::Ref{CFpOut}) -> code, into (sum, sumsq, nused, n) with sum and sumsq W × M × U; `channels` is
# empty (all C channels in order) or M × U 0-based block channels, -1 for an empty slot
function _fp_run(call, U, C, pre, W, channels::Matrix{Int32})
    isempty(channels) || size(channels, 2) == U || error("footprints: channels needs one column per unit")
    M = isempty(channels) ? C : size(channels, 1)
    s = zeros(Float64, W, M, U); q = zeros(Float64, W, M, U); nused = zeros(Int64, U); n = zeros(Int64, U)
    GC.@preserve channels s q nused n begin
        check(call(Ref(CFpOpt(pre, W, M, isempty(channels) ? C_NULL : pointer(channels))),
                   Ref(CFpOut(pointer(s), pointer(q), pointer(nused), pointer(n)))))
    end
    (sum=s, sumsq=q, nused=nused, n=n)
end

"""
    footprints(block, times; pre=20, W=60, channels=zeros(Int32, 0, 0)) -> (sum, sumsq, nused, n)

Spike-triggered sum and sum of squares of every unit on every channel of a block (`hmmsort_footprints`; an extension,
INTEGRATION.md "Footprints"): `block` is samples × channels (column-major, so channel-major in memory) of Float64 or
Int16 samples, `times` one ascending vector of 1-based spike times per unit.  `sum[k, m, u]` adds `block[t - pre + k - 1, c]`
over the spikes `t` of unit `u` whose window lies inside the block, `c` being channel `m` or `channels[m, u] + 1`;
`sum ./ nused` is the unit's mean waveform on every channel.  The order of the adds is fixed (include/hmmsort.h).
"""
function footprints(block::Matrix{T}, times::Vector{Vector{Int64}}; pre::Integer=20, W::Integer=60,
                    channels::Matrix{Int32}=zeros(Int32, 0, 0)) where T <: Union{Float64,Int16}
    n, C = size(block); U = length(times)
    ptrs = [isempty(t) ? Ptr{Int64}(C_NULL) : pointer(t) for t in times]; counts = Int64.(length.(times))
    GC.@preserve block times ptrs counts begin
        _fp_run(U, C, pre, W, channels) do opt, out
            ccall((:hmmsort_footprints, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Ptr{Int64}}, Ptr{Int64}, Ref{CFpOpt}, Ref{CFpOut}),
                block, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, C, n, U, ptrs, counts, opt, out)
        end
    end
end

"`footprints` of a resident `[C][n]` Float64 block and spike lists concatenated in device memory behind the `U + 1` host offsets `offs` (`hmmsort_footprints_device`); synchronises `stream`"
function footprints_device(d_y::Ptr{Float64}, C::Integer, n::Integer, d_times::Ptr{Int64}, offs::Vector{Int64};
                           pre::Integer=20, W::Integer=60, channels::Matrix{Int32}=zeros(Int32, 0, 0),
                           stream::Ptr{Cvoid}=C_NULL)
    U = length(offs) - 1
    GC.@preserve offs begin
        _fp_run(U, C, pre, W, channels) do opt, out
            ccall((:hmmsort_footprints_device, lib), Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{CFpOpt}, Ref{CFpOut}, Ptr{Cvoid}),
                d_y, C, n, U, d_times, offs, opt, out, stream)
        end
    end
end

"`footprints` of the units `u = ch N + a` a plan finds on its resident path(s) `d_x`, on every channel of the resident `[Cb][n]` Float64 block `d_block` of the plan's length (`hmmsort_plan_footprints`); `U` = the plan's channels × templates; synchronises `stream`"
function footprints_plan(plan::Ptr{Cvoid}, d_x::Ptr{Int16}, d_block::Ptr{Float64}, Cb::Integer, U::Integer;
                         pre::Integer=20, W::Integer=60, channels::Matrix{Int32}=zeros(Int32, 0, 0),
                         stream::Ptr{Cvoid}=C_NULL)
    _fp_run(U, Cb, pre, W, channels) do opt, out
        ccall((:hmmsort_plan_footprints, lib), Cint,
            (Ptr{Cvoid}, Ptr{Int16}, Ptr{Float64}, Int64, Ref{CFpOpt}, Ref{CFpOut}, Ptr{Cvoid}),
            plan, d_x, d_block, Cb, opt, out, stream)
    end
end

# struct hmmsort_feat_opt / hmmsort_feat_out / hmmsort_iso_out (include/hmmsort.h)
struct CFeatOpt
    pre::Int64; W::Int64; M::Int64; chan::Ptr{Int32}; P::Int64; basis::Ptr{Float64}; centre::Ptr{Float64}; moments::Int64
end
struct CFeatOut
    feat::Ptr{Float64}; used::Ptr{UInt8}; cap_rows::Int64; n::Ptr{Int64}; nused::Ptr{Int64}
    b1::Ptr{Float64}; b2::Ptr{Float64}; g1::Ptr{Float64}; g2::Ptr{Float64}
end
struct CIsoOut
    iso_d2::Ptr{Float64}; closer::Ptr{Int64}; lpair::Ptr{Float64}
end

# call(opt::Ref{CFeatOpt}, out::Ref{CFeatOut}) -> code.  `channels`: empty (all C channels in order) or the 0-based block
# channels of the M slots, one row for all units; `basis` W × P × M (empty: none, P := W), `centre` W × M (empty: zeros);
# feat / used: where the rows go (host arrays in the host form, device memory otherwise; C_NULL: no rows), cap_rows what
# they hold.  Moments come back column-major: b1 P × M × U, b2 P × P × M × U, g1 F × U, g2 F × F × U.
function _feat_run(call, U, C, pre, W, channels::Vector{Int32}, basis::Array{Float64,3}, centre::Matrix{Float64},
                   moments, feat, used, cap_rows)
    M = isempty(channels) ? C : length(channels)
    P = isempty(basis) ? W : size(basis, 2)
    F = M * P
    n = zeros(Int64, U); nused = zeros(Int64, U)
    b1 = moments == 1 ? zeros(Float64, P, M, U) : zeros(Float64, 0, 0, 0)
    b2 = moments == 1 ? zeros(Float64, P, P, M, U) : zeros(Float64, 0, 0, 0, 0)
    g1 = moments == 2 ? zeros(Float64, F, U) : zeros(Float64, 0, 0)
    g2 = moments == 2 ? zeros(Float64, F, F, U) : zeros(Float64, 0, 0, 0)
    nul(a) = isempty(a) ? Ptr{eltype(a)}(C_NULL) : pointer(a)
    GC.@preserve channels basis centre n nused b1 b2 g1 g2 begin
        check(call(Ref(CFeatOpt(pre, W, M, nul(channels), isempty(basis) ? 1 : P, nul(basis), nul(centre), moments)),
                   Ref(CFeatOut(feat, used, cap_rows, pointer(n), pointer(nused), nul(b1), nul(b2), nul(g1), nul(g2)))))
    end
    (n=n, nused=nused, b1=b1, b2=b2, g1=g1, g2=g2, F=F)
end

"""
    snippet_features(block, times; pre=20, W=60, channels=Int32[], basis, centre, moments=0, rows=true)
        -> (features, used, n, nused, b1, b2, g1, g2)

One feature row per spike (`hmmsort_snippet_features`; an extension, INTEGRATION.md "Isolation"): `block` and `times` as
`footprints` takes them; `features` is F × n_total (row `r` of the C layout is column `r`), rows in unit order.  Without
a basis the row is the spike's snippets on the listed channels minus `centre`; with `basis` (W × P × M) the P
projections per channel.  `moments`: 1 the per-channel sums for the PCA, 2 the per-unit sums over whole rows.
"""
function snippet_features(block::Matrix{T}, times::Vector{Vector{Int64}}; pre::Integer=20, W::Integer=60,
                          channels::Vector{Int32}=Int32[], basis::Array{Float64,3}=zeros(Float64, 0, 0, 0),
                          centre::Matrix{Float64}=zeros(Float64, 0, 0), moments::Integer=0,
                          rows::Bool=true) where T <: Union{Float64,Int16}
    n, C = size(block); U = length(times)
    ptrs = [isempty(t) ? Ptr{Int64}(C_NULL) : pointer(t) for t in times]; counts = Int64.(length.(times))
    M = isempty(channels) ? C : length(channels)
    F = M * (isempty(basis) ? W : size(basis, 2)); total = sum(counts)
    feat = rows ? zeros(Float64, F, total) : zeros(Float64, 0, 0); used = rows ? zeros(UInt8, total) : UInt8[]
    GC.@preserve block times ptrs counts feat used begin
        r = _feat_run(U, C, pre, W, channels, basis, centre, moments,
                      rows ? pointer(feat) : Ptr{Float64}(C_NULL), rows ? pointer(used) : Ptr{UInt8}(C_NULL), total) do opt, out
            ccall((:hmmsort_snippet_features, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Ptr{Int64}}, Ptr{Int64}, Ref{CFeatOpt}, Ref{CFeatOut}),
                block, T === Int16 ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, C, n, U, ptrs, counts, opt, out)
        end
    end
    (features=feat, used=used, n=r.n, nused=r.nused, b1=r.b1, b2=r.b2, g1=r.g1, g2=r.g2)
end

"`snippet_features` of a resident `[C][n]` Float64 block and resident lists (`hmmsort_snippet_features_device`); `d_feat` / `d_used`: device memory for `offs[end] - offs[1]` rows, or `C_NULL`; synchronises `stream`"
function snippet_features_device(d_y::Ptr{Float64}, C::Integer, n::Integer, d_times::Ptr{Int64}, offs::Vector{Int64};
                                 pre::Integer=20, W::Integer=60, channels::Vector{Int32}=Int32[],
                                 basis::Array{Float64,3}=zeros(Float64, 0, 0, 0),
                                 centre::Matrix{Float64}=zeros(Float64, 0, 0), moments::Integer=0,
                                 d_feat::Ptr{Float64}=Ptr{Float64}(C_NULL), d_used::Ptr{UInt8}=Ptr{UInt8}(C_NULL),
                                 stream::Ptr{Cvoid}=C_NULL)
    U = length(offs) - 1
    GC.@preserve offs begin
        _feat_run(U, C, pre, W, channels, basis, centre, moments, d_feat, d_used, offs[end] - offs[1]) do opt, out
            ccall((:hmmsort_snippet_features_device, lib), Cint,
                (Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{CFeatOpt}, Ref{CFeatOut}, Ptr{Cvoid}),
                d_y, C, n, U, d_times, offs, opt, out, stream)
        end
    end
end

"`snippet_features` of the units `u = ch N + a` a plan finds on its resident path(s) `d_x` (`hmmsort_plan_snippet_features`); a first call without rows returns `n`; `cap_rows` is what `d_feat` / `d_used` hold (fewer than `sum(n)`: no row is written); synchronises `stream`"
function snippet_features_plan(plan::Ptr{Cvoid}, d_x::Ptr{Int16}, d_block::Ptr{Float64}, Cb::Integer, U::Integer;
                               pre::Integer=20, W::Integer=60, channels::Vector{Int32}=Int32[],
                               basis::Array{Float64,3}=zeros(Float64, 0, 0, 0),
                               centre::Matrix{Float64}=zeros(Float64, 0, 0), moments::Integer=0,
                               d_feat::Ptr{Float64}=Ptr{Float64}(C_NULL), d_used::Ptr{UInt8}=Ptr{UInt8}(C_NULL),
                               cap_rows::Integer=0, stream::Ptr{Cvoid}=C_NULL)
    _feat_run(U, Cb, pre, W, channels, basis, centre, moments, d_feat, d_used, cap_rows) do opt, out
        ccall((:hmmsort_plan_snippet_features, lib), Cint,
            (Ptr{Cvoid}, Ptr{Int16}, Ptr{Float64}, Int64, Ref{CFeatOpt}, Ref{CFeatOut}, Ptr{Cvoid}),
            plan, d_x, d_block, Cb, opt, out, stream)
    end
end

"""
    cluster_isolation(features, offs, mu, Vinv; used=UInt8[]) -> (iso_d2, closer, lpair)

`hmmsort_cluster_isolation`: `features` F × n (column `r` is row `r`), `offs` the U + 1 0-based row offsets, `mu` F × U,
`Vinv` F × F × U with `Vinv[b, a, u]` the C entry `[u][a][b]` (a unit whose `Vinv[1, 1, u]` is NaN is not scored).
`closer[v, u]` and `lpair[v, u]` are the C entries `[u][v]`.
"""
function cluster_isolation(features::Matrix{Float64}, offs::Vector{Int64}, mu::Matrix{Float64}, Vinv::Array{Float64,3};
                           used::Vector{UInt8}=UInt8[])
    F, n = size(features); U = length(offs) - 1
    d2 = zeros(Float64, U); closer = zeros(Int64, U, U); lpair = zeros(Float64, U, U)
    GC.@preserve features offs mu Vinv used d2 closer lpair begin
        check(ccall((:hmmsort_cluster_isolation, lib), Cint,
            (Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ref{CIsoOut}),
            features, n, F, U, offs, isempty(used) ? Ptr{UInt8}(C_NULL) : pointer(used), mu, Vinv,
            Ref(CIsoOut(pointer(d2), pointer(closer), pointer(lpair)))))
    end
    (iso_d2=d2, closer=closer, lpair=lpair)
end

"`cluster_isolation` on resident rows `d_feat` (`[n][F]`) and used bytes `d_used` (or `C_NULL`) (`hmmsort_cluster_isolation_device`); synchronises `stream`"
function cluster_isolation_device(d_feat::Ptr{Float64}, n::Integer, F::Integer, offs::Vector{Int64}, mu::Matrix{Float64},
                                  Vinv::Array{Float64,3}; d_used::Ptr{UInt8}=Ptr{UInt8}(C_NULL),
                                  stream::Ptr{Cvoid}=C_NULL)
    U = length(offs) - 1
    d2 = zeros(Float64, U); closer = zeros(Int64, U, U); lpair = zeros(Float64, U, U)
    GC.@preserve offs mu Vinv d2 closer lpair begin
        check(ccall((:hmmsort_cluster_isolation_device, lib), Cint,
            (Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ref{CIsoOut}, Ptr{Cvoid}),
            d_feat, n, F, U, offs, d_used, mu, Vinv, Ref(CIsoOut(pointer(d2), pointer(closer), pointer(lpair))), stream))
    end
    (iso_d2=d2, closer=closer, lpair=lpair)
end

# struct hmmsort_stab_opt / hmmsort_stab_out (include/hmmsort.h)
struct CStabOpt
    T::Int64; bin::Int64; nq::Int64; q_num::NTuple{8,Int64}; q_den::Int64; HB::Int64; hist_lo::Float64; hist_scale::Float64
end
struct CStabOut
    n::Ptr{Int64}; count::Ptr{Int64}; valid::Ptr{Int64}; quant::Ptr{Float64}; sum::Ptr{Float64}; sumsq::Ptr{Float64}
    uvalid::Ptr{Int64}; uquant::Ptr{Float64}; umin::Ptr{Float64}; umax::Ptr{Float64}; usum::Ptr{Float64}
    usumsq::Ptr{Float64}; hist::Ptr{Int64}; under::Ptr{Int64}; over::Ptr{Int64}
end

# call(opt::Ref{CStabOpt}, out::Ref{CStabOut}) -> code, into a named tuple of the tables; arrays are column-major, so
# count is B × U, quant nq × B × U, hist HB × U.  `quantiles` are exact rationals (q_num = q .* q_den), `hist` is
# nothing or (bins, lo, scale)
function _stab_run(call, U, n, bin, quantiles::Vector{<:Rational}, hist)
    nq = length(quantiles); nq <= 8 || error("unit_stability: at most 8 quantiles")
    q_den = nq == 0 ? 1 : lcm(denominator.(quantiles)...)
    q_num = ntuple(k -> k <= nq ? Int64(numerator(quantiles[k]) * (q_den ÷ denominator(quantiles[k]))) : Int64(0), 8)
    HB, lo, scale = hist === nothing ? (0, 0.0, 1.0) : hist
    B = cld(n, bin)
    cnt = zeros(Int64, B, U); valid = zeros(Int64, B, U); quant = zeros(Float64, nq, B, U)
    s = zeros(Float64, B, U); q = zeros(Float64, B, U); nn = zeros(Int64, U); uvalid = zeros(Int64, U)
    uquant = zeros(Float64, nq, U); umin = zeros(Float64, U); umax = zeros(Float64, U); usum = zeros(Float64, U)
    usumsq = zeros(Float64, U); h = zeros(Int64, HB, U); under = zeros(Int64, U); over = zeros(Int64, U)
    GC.@preserve cnt valid quant s q nn uvalid uquant umin umax usum usumsq h under over begin
        check(call(Ref(CStabOpt(n, bin, nq, q_num, q_den, HB, lo, scale)),
                   Ref(CStabOut(pointer(nn), pointer(cnt), pointer(valid), pointer(quant), pointer(s), pointer(q),
                                pointer(uvalid), pointer(uquant), pointer(umin), pointer(umax), pointer(usum),
                                pointer(usumsq), pointer(h), pointer(under), pointer(over)))))
    end
    (n=nn, count=cnt, valid=valid, quant=quant, sum=s, sumsq=q, uvalid=uvalid, uquant=uquant, umin=umin, umax=umax,
     usum=usum, usumsq=usumsq, hist=h, under=under, over=over)
end

"""
    unit_stability(times, values, n; bin, quantiles=[1//4, 1//2, 3//4], hist=nothing) -> named tuple of tables

Spike counts per unit and time bin of `bin` samples of a recording of `n` samples and, of one Float64 value per spike
(NaN: no value), exact order statistics, sums and a histogram per unit and bin and per unit (`hmmsort_unit_stability`; an
extension, INTEGRATION.md "Stability").  `times` is one ascending vector of 1-based spike times per unit, `values` one
vector per unit of the same lengths or `nothing` for the counts alone (the other tables then stay zero).  A quantile is
the value of rank `floor(q (m - 1))` among the `m` values of a bin, never interpolated.
"""
function unit_stability(times::Vector{Vector{Int64}}, values::Union{Nothing,Vector{Vector{Float64}}}, n::Integer;
                        bin::Integer, quantiles::Vector{<:Rational}=[1//4, 1//2, 3//4], hist=nothing)
    U = length(times)
    ptrs = [isempty(t) ? Ptr{Int64}(C_NULL) : pointer(t) for t in times]; counts = Int64.(length.(times))
    vptrs = values === nothing ? Ptr{Float64}[] : [isempty(v) ? Ptr{Float64}(C_NULL) : pointer(v) for v in values]
    GC.@preserve times values ptrs vptrs counts begin
        _stab_run(U, n, bin, quantiles, hist) do opt, out
            ccall((:hmmsort_unit_stability, lib), Cint,
                (Int64, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ref{CStabOpt}, Ref{CStabOut}),
                U, ptrs, values === nothing ? C_NULL : vptrs, counts, opt, out)
        end
    end
end

"`unit_stability` of spike lists and values concatenated in device memory behind the `U + 1` host offsets `offs` (`hmmsort_unit_stability_device`; `d_values` may be `C_NULL`); synchronises `stream`"
function unit_stability_device(d_times::Ptr{Int64}, d_values::Ptr{Float64}, offs::Vector{Int64}, n::Integer;
                               bin::Integer, quantiles::Vector{<:Rational}=[1//4, 1//2, 3//4], hist=nothing,
                               stream::Ptr{Cvoid}=C_NULL)
    U = length(offs) - 1
    GC.@preserve offs begin
        _stab_run(U, n, bin, quantiles, hist) do opt, out
            ccall((:hmmsort_unit_stability_device, lib), Cint,
                (Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ref{CStabOpt}, Ref{CStabOut}, Ptr{Cvoid}),
                U, d_times, d_values, offs, opt, out, stream)
        end
    end
end

"`unit_stability` of the units `u = ch N + a` a plan finds on its resident path(s) `d_x`, with the amplitude `hmmsort_plan_spike_fit` gives every event on the resident signal(s) `d_y` as its value (`hmmsort_plan_unit_stability`); `n` is the plan's length, `U` its channels × templates; synchronises `stream`"
function unit_stability_plan(plan::Ptr{Cvoid}, d_y::Ptr{Float64}, d_x::Ptr{Int16}, n::Integer, U::Integer;
                             bin::Integer, quantiles::Vector{<:Rational}=[1//4, 1//2, 3//4], hist=nothing,
                             stream::Ptr{Cvoid}=C_NULL)
    _stab_run(U, n, bin, quantiles, hist) do opt, out
        ccall((:hmmsort_plan_unit_stability, lib), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int16}, Ref{CStabOpt}, Ref{CStabOut}, Ptr{Cvoid}),
            plan, d_y, d_x, opt, out, stream)
    end
end

function reconstruct_signal(x::Array{T,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) where T <: Integer
    xs = T === Int16 ? x : Int16.(x)
    Y2 = zeros(Float64, length(xs))
    check(ccall((:hmmsort_reconstruct, lib), Cint,
        (Ptr{Int16}, Int64, Ptr{Int16}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
        xs, length(xs), lA.states, lA.N, lA.nstates, μ, size(μ, 1), Y2))
    Y2
end

"""
    posteriors(y, lA, μ, σ; decode=false) -> (onset, occ, silent, xm, logz)

Smoothed state posteriors (an extension, no counterpart in the reference; INTEGRATION.md "Posteriors"):
`onset[t, a]` / `occ[t, a]` = posterior that template `a` is at its first phase / mid-spike at sample `t`,
`silent[t]` that of the silent state, `logz` the log-likelihood of the recording; with `decode=true`, `xm[t]` =
the state of largest posterior (1-based, like `viterbi`'s path), else `xm` is empty.
"""
function posteriors(y::AbstractArray{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64; decode=false)
    yv = y isa Array ? y : collect(y)
    T = length(yv)
    onset = zeros(Float64, T, lA.N); occ = zeros(Float64, T, lA.N); silent = zeros(Float64, T)
    xm = zeros(Int16, decode ? T : 0); logz = Ref{Float64}(0.0)
    check(ccall((:hmmsort_posteriors, lib), Cint,
        (Ptr{Float64}, Int64, Ptr{Int16}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int16}, Ref{Float64}),
        yv, T, lA.states, lA.N, lA.K, lA.nstates, lA.transitions, length(lA.transitions), μ, σ,
        onset, occ, silent, decode ? pointer(xm) : Ptr{Int16}(C_NULL), logz))
    onset, occ, silent, xm, logz[]
end

"Free the plans and device buffers the library keeps between host-buffer calls."
shutdown() = check(ccall((:hmmsort_shutdown, lib), Cint, ()))
set_option(key::String, value::Integer) = check(ccall((:hmmsort_set_option, lib), Cint, (Cstring, Int64), key, value))

"Replace the reference's method bodies by the GPU versions (same signatures)."
function enable!()
    @eval HMMSpikeSorter begin
        viterbi(y::AbstractArray{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = $(viterbi)(y, lA, μ, σ)
        viterbi(y::AbstractArray{Int16,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = $(viterbi)(y, lA, μ, σ)
        forward(V::Array{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = $(forward)(V, lA, μ, σ)
        backward(V::Array{Float64,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) = $(backward)(V, lA, μ, σ)
        update(α::Array{Float64,2}, β::Array{Float64,2}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64, x::Array{Float64,1}) = $(update)(α, β, lA, μ, σ, x)
        train_model(X::Array{Float64,1}, sm::StateMatrix, μ0::Array{Float64,2}, σ0::Float64; verbose=0) = $(train_model)(X, sm, μ0, σ0; verbose=verbose)
        reconstruct_signal(x::Array{T,1}, lA::StateMatrix, μ::Array{Float64,2}, σ::Float64) where T <: Integer = $(reconstruct_signal)(x, lA, μ, σ)
        StatsBase.fit(::Type{HMMSpikingModel}, templates::HMMSpikeTemplateModel, X::AbstractVector{Float64}, chunksize::Integer, callback::Function=x->nothing) = $(fit_chunked)(templates, X, chunksize)
    end
    atexit(shutdown)
    nothing
end

end # module
