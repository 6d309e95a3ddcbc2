# AGPHip.jl -- Julia shim over libagp_hip.so (include/agp_hip.h).
#
# NOT EXECUTED IN THE BUILD ENVIRONMENT (no julia binary there or on the GPU box); it is the binding a maintainer of
# AugmentedGaussianProcesses.jl would add so that SVGP / MOSVGP models with AnalyticVI / AnalyticSVI run their hot path on an
# MI355X, written against the reference's own internals (file:line cited at every method).  AMDGPU.jl is used ONLY for device /
# stream / buffer handles (ROCArray, the stream pointer); there is no KernelAbstractions and no CUDA.jl compatibility layer:
# every numeric operation is a `ccall` into hand-written HIP.
#
# Usage -- the reference API, unchanged, on the reference's own model objects (section "drop-in methods" at the end):
#
#     using AugmentedGaussianProcesses, AGPHip                                              # loading the shim is the switch
#     m = SVGP(kernel, LogisticLikelihood(), AnalyticSVI(1024), Z; optimiser=false)        # the reference constructor
#     m, state = train!(m, X, y, 1000)                  # src/training/training.jl:13-111, now on the MI355X (backend=:cpu opts out)
#     ŷ = predict_y(m, X_test); p = proba_y(m, X_test); μ, σ² = predict_f(m, X_test; cov=true); ELBO(m, X, y)
#     Z = AGPHip.inducingpoints(KmeansAlg(1024), X)      # the device k-means (agp_kmeans) behind InducingPoints' interface
#     om = OnlineSVGP(kernel, GaussianLikelihood(), AnalyticVI(), OIPS(0.9)); train!(om, Xbatch, ybatch; iterations=5)
#
# The explicit form (a wrapped model, for multi-GPU runs and for tests that keep both paths side by side) is still there:
#     hm = AGPHip.HipModel(m); hm, state = train!(hm, X, y, 1000); predict_y(hm, X_test); ELBO(hm, X, y); objective(hm, state, y)
#
# Seams replaced (SURVEY.md section 8b):
#   update_parameters!(model::SVGP / ::MOSVGP, state, x, y)   src/training/training.jl:140-158        -> agp_svgp_cavi_step[_multi]
#   compute_K / compute_κ                                     src/gpblocks/latentgp.jl:205-215         -> inside the step / agp_svgp_refresh_K
#   update_hyperparameters!(m, state, x, y)                   src/hyperparameter/autotuning.jl:86-140  -> agp_svgp_hyper_step[_multi]
#   ELBO(model, state, y) / ELBO(model, X, y)                 src/inference/analyticVI.jl:255-297, src/functions/ELBO.jl:32-47 -> agp_svgp_elbo
#   ELBO(model, X, y; streamed=true)                          the same over any number of points                   -> agp_svgp_elbo_stream
#   log_predictive_density(model, X, y) (no counterpart: the held-out log-likelihood / NLPD)           -> agp_svgp_lpd_stream, agp_log_predictive
#   _predict_f / predict_y / proba_y                          src/training/predictions.jl:25-92,178-247 -> agp_svgp_predict_f / _predict_y / _proba_y
#   predict_f_grad(model, X_test) (no counterpart: d mu / d x*, d sigma^2 / d x* of predict_f)          -> agp_svgp_predict_f_grad
#   acquisition / maximize_acquisition(model, UCB | EI | PI | LogEI | LogPI, ...) (no counterpart: Bayesian optimisation) -> agp_svgp_acquisition, agp_svgp_acq_maximize
#   acquisition_pending / maximize_acquisition_batch(model, ...; pending) (no counterpart: batch acquisition by hallucinated
#     observations)                                                                  -> agp_svgp_acquisition_pending, agp_svgp_acq_maximize_batch
#   acquisition_joint / maximize_acquisition_joint(model, EI | UCB, ...) (no counterpart: Monte-Carlo q-EI / q-UCB with a joint
#     reparameterised sample)                                                        -> agp_svgp_acquisition_joint, agp_svgp_acq_maximize_joint
#   init_state                                                src/training/states.jl:1-9               -> agp_svgp_init_state
# Multi-GPU (one Julia process per GPU, e.g. under MPI.jl or Distributed): agp_comm_* binds RCCL inside the library; the host only
# ships the 128-byte id from rank 0 to the others (section "multi-GPU" below).
module AGPHip

using AMDGPU
using AugmentedGaussianProcesses
using KernelFunctions
using LinearAlgebra
using StatsBase: sample, Weights
import StatsBase: sample               # (extended for MCGP below)
using Random
using Optimisers
import ProgressMeter                      # (a dependency of the reference: train!'s progress reporting, training.jl:46,71-90)
const AGP = AugmentedGaussianProcesses

import AugmentedGaussianProcesses: train!, predict_f, predict_y, proba_y, ELBO, objective

const libagp = get(ENV, "AGP_HIP_LIB", joinpath(@__DIR__, "..", "augmentedgaussianprocesses.jl_amd", "libagp_hip.so"))

# ---- POD mirrors of include/agp_hip.h (field order and widths are checked by tests/test_host_abi.py on the Python mirror) -------
struct KernelDesc
    kind::Int32
    ard::Int32
    variance::Float64
    scale::Float64
    ard_scales_host::Ptr{Float64}
    has_variance::Int32          # the kernel object is `σ² * k`            (what update_kernel! may step,
    has_transform::Int32         # the kernel object is `k ∘ Scale/ARDTransform`   autotuning_utils.jl:47-67)
end
struct LikDesc
    kind::Int32
    n_class::Int32
    p0::Float64
    p1::Float64
end
struct SvgpDesc
    dtype::Int32
    n_latent::Int32
    latent_offset::Int32
    stochastic::Int32
    m::Int64
    D::Int64
    max_batch::Int64
    lik::LikDesc
    jitter::Float64
    rm_kappa::Float64
    rm_tau::Float64
    elbo_mode::Int32
    flags::Int32                 # AGP_FLAG_STALE_K = 1 : reference_compat_stale_K (training.jl:187-208, SURVEY Appendix A Q1)
end
const AGP_FLAG_STALE_K = Int32(1)
const AGP_FLAG_FULL = Int32(2)     # VGP: the full model, kappa = I, m = N, Z = the training inputs (agp_hip.h)
const AGP_FLAG_EXACT = Int32(4)    # GP: exact regression with Analytic(), together with AGP_FLAG_FULL (agp_hip.h)
const AGP_FLAG_SAMPLED = Int32(8)  # MCGP: Gibbs sampling of the augmented full model, together with AGP_FLAG_FULL (agp_hip.h)
const AGP_FLAG_NUMERICAL = Int32(16)  # QuadratureVI (with AGP_FLAG_FULL: VGP; alone: SVGP): the handle keeps (mu, Sigma) and the optimiser's moments (agp_hip.h)
const AGP_FLAG_MC = Int32(32)  # MCIntegrationVI over K latents, together with AGP_FLAG_NUMERICAL (agp_hip.h, "MC INTEGRATION")
const AGP_LIK_SOFTMAX = Int32(10)  # SoftMaxLikelihood(K): no augmentation, AGP_FLAG_MC handles only (softmax.jl)
const AGP_SHARD_LATENT, AGP_SHARD_BATCH = Int32(0), Int32(1)

struct AGPError <: Exception
    status::Int32
    msg::String
end
function check(ctx, st::Integer)
    st == 0 && return nothing
    msg = unsafe_string(ccall((:agp_last_error, libagp), Cstring, (Ptr{Cvoid},), ctx))
    if st == 2                                                   # cholesky failure, latentgp.jl:206
        mt = match(r"leading minor (\d+)", msg)
        throw(PosDefException(mt === nothing ? 0 : parse(Int, mt.captures[1])))
    end
    st == 3 && error("K̃ has negative values")                    # latentgp.jl:213
    st == 4 && error(msg)                                        # batch-size check, training.jl:27-29
    st == 6 && throw(ArgumentError(msg))                         # treat_labels!, classification.jl:36-44 / multiclass.jl:81-83
    throw(AGPError(Int32(st), msg))
end

# ---- KernelFunctions.jl objects -> agp_kernel_desc ----------------------------------------------------------------------------
kind(::SqExponentialKernel) = Int32(0)
kind(::Matern52Kernel) = Int32(1)
kind(::Matern32Kernel) = Int32(2)
kind(::ExponentialKernel) = Int32(3)
function kernel_desc(k::Kernel, D::Int)
    σ², hasv = 1.0, Int32(0)
    if k isa ScaledKernel
        σ² = only(k.σ²); k = k.kernel; hasv = Int32(1)
    end
    if k isa TransformedKernel
        t = k.transform; b = k.kernel
        if t isa ScaleTransform
            return KernelDesc(kind(b), 0, σ², only(t.s), C_NULL, hasv, 1), nothing
        elseif t isa ARDTransform
            v = Vector{Float64}(t.v)
            length(v) == D || throw(DimensionMismatch("ARDTransform has $(length(v)) scales, the data $D dimensions"))
            return KernelDesc(kind(b), 1, σ², 1.0, pointer(v), hasv, 1), v   # keep v alive (GC.@preserve at the call)
        end
        error("only ScaleTransform / ARDTransform are wired on the HIP path")
    end
    return KernelDesc(kind(k), 0, σ², 1.0, C_NULL, hasv, 0), nothing
end

# write the (possibly optimised) parameters back into the reference's kernel object (what update_kernel! mutates in place)
function pull_kernel!(k::Kernel, σ²::Float64, scales::Vector{Float64})
    if k isa ScaledKernel
        k.σ² .= σ²; k = k.kernel
    end
    if k isa TransformedKernel
        t = k.transform
        t isa ScaleTransform && (t.s .= scales[1])
        t isa ARDTransform && (t.v .= scales)
    end
    return nothing
end

# opt_noise (gaussian.jl:18-23): p1 carries the ADAM learning rate, σ² is then device state (pull_hypers! mirrors it back)
lik_desc(l::GaussianLikelihood) = LikDesc(0, 1, AGP.noise(l), l.opt_noise === nothing ? 0.0 : Float64(l.opt_noise.eta))
lik_desc(::AGP.BernoulliLikelihood{<:AGP.LogisticLink}) = LikDesc(1, 1, 0.0, 0.0)
lik_desc(l::StudentTLikelihood) = LikDesc(2, 1, l.ν, l.σ)
lik_desc(l::AGP.MultiClassLikelihood{<:AGP.LogisticSoftMaxLink}) = LikDesc(3, AGP.n_class(l), 0.0, 0.0)
lik_desc(l::LaplaceLikelihood) = LikDesc(5, 1, l.β, 0.0)
lik_desc(::AGP.BernoulliLikelihood{<:AGP.SVMLink}) = LikDesc(6, 1, 0.0, 0.0)
lik_desc(l::AGP.PoissonLikelihood{<:AGP.ScaledLogistic}) = LikDesc(7, 1, only(l.invlink.λ), 0.0)   # λ is state: pull_lik_state!
lik_desc(l::NegBinomialLikelihood) = LikDesc(8, 1, Float64(l.r), 0.0)
lik_desc(l::AGP.HeteroscedasticGaussianLikelihood{<:AGP.InvScaledLogistic}) = LikDesc(9, 1, only(l.invlink.λ), 0.0)
lik_desc(l) = error("The $l is not compatible or implemented with AnalyticVI on the HIP path")     # SVGP.jl:48-49

is_multiclass(l) = l isa AGP.MultiClassLikelihood
is_bernoulli(l) = l isa AGP.BernoulliLikelihood
is_event(l) = l isa AGP.PoissonLikelihood || l isa NegBinomialLikelihood

# ---- the device twin of a reference model -------------------------------------------------------------------------------------
mutable struct HipModel{T,M<:AGP.AbstractGPModel{T}}
    model::M                       # the reference object: kernels, Z, likelihood, inference, posterior live on in it
    ctx::Ptr{Cvoid}
    h::Ptr{Cvoid}
    comm::Ptr{Cvoid}               # agp_comm* (C_NULL: single GPU)
    shard::Int32                   # AGP_SHARD_LATENT / AGP_SHARD_BATCH when comm is set
    latent_range::UnitRange{Int}   # latents of model.f held by this rank (all of them unless latent-parallel)
    maxbatch::Int
    X::Union{Nothing,ROCMatrix{T}} # D x N (ColVecs memory order == the ABI's point-major layout)
    y::Any                         # ROCVector{T} / ROCVector{Int32} (class index) / ROCMatrix{T} (n_task x N, multi-output)
    N::Int
    last_idx::Any                  # device indices of the last minibatch (kept alive: the step is asynchronous)
    stale_K::Bool
    rank::Int32                    # place in a multi-GPU run (comm_init!): re-applied whenever the handle is re-created
    world::Int32
    keep::Vector{Any}              # index buffers a queued look-ahead / pending step may still read (two generations)
end

is_mo(hm::HipModel) = hm.model isa Union{AGP.MOSVGP,AGP.MOVGP}
is_full(hm::HipModel) = hm.model isa Union{AGP.VGP,AGP.GP,AGP.MOVGP,AGP.MCGP}   # (a MOVGP is both: IsMultiOutput and IsFull, MOVGP.jl:121-122)
is_exact(hm::HipModel) = hm.model isa AGP.GP
is_sampled(hm::HipModel) = hm.model isa AGP.MCGP
is_numerical(hm::HipModel) = hm.model isa Union{AGP.VGP,SVGP} && AGP.inference(hm.model) isa AGP.QuadratureVI
# the latents of a model: a tuple / vector of them (SVGP, MOSVGP, VGP, MOVGP: `m.f`), or the single LatentGP of a GP (`f::LatentGP`, GP.jl:28)
latents(m::AGP.AbstractGPModel) = m.f
latents(m::AGP.GP) = (m.f,)
# the inputs the handle's "inducing points" are: Z of a sparse latent, the training inputs of a VGP (Zviews(m::VGP), VGP.jl:90)
zview(hm::HipModel, gp) = is_full(hm) ? AGP.input(hm.model.data) : AGP.Zview(gp)
nlat(hm::HipModel) = length(hm.latent_range)

"""
    HipModel(model::Union{SVGP,MOSVGP}; device=AMDGPU.device_id()-1, reference_compat_stale_K=false,
             latent_range=1:length(latents(model)))

Wrap a reference model.  Nothing is allocated on the device until data arrive (`train!`, `ELBO`, `predict_*`).
"""
function HipModel(model::M; reference_compat_stale_K::Bool=false,
                  latent_range::UnitRange{Int}=1:length(latents(model))) where {T,M<:AGP.AbstractGPModel{T}}
    model isa Union{SVGP,AGP.MOSVGP,AGP.VGP,AGP.GP,AGP.MOVGP,AGP.MCGP} ||
        error("only SVGP / MOSVGP / VGP / GP / MOVGP / MCGP run on the HIP path")
    model isa Union{AGP.VGP,AGP.GP,AGP.MOVGP,AGP.MCGP} && T != Float64 && error("VGP / GP / MOVGP / MCGP run in Float64 only on the HIP path")
    AGP.inference(model) isa (model isa AGP.MCGP ? AGP.GibbsSampling :
                              model isa Union{AGP.VGP,SVGP} ? Union{AnalyticVI,AGP.QuadratureVI} : Union{AnalyticVI,AGP.Analytic}) ||
        error("The inference object should be of type `AnalyticVI` (MCGP: `GibbsSampling`; SVGP and VGP also take `QuadratureVI`)")   # SVGP.jl:45-47, MCGP.jl:51-53
    if model isa Union{AGP.VGP,SVGP} && AGP.inference(model) isa AGP.QuadratureVI   # what the numerical handle refuses (agp_hip.h, "NUMERICAL INFERENCE")
        model isa AGP.VGP && AGP.is_stochastic(AGP.inference(model)) && error("VGP takes the full data set every iteration: use QuadratureVI()")
        model isa SVGP && any(gp -> AGP.Zopt(gp) !== nothing, latents(model)) && error("SVGP with QuadratureVI: the inducing points are not optimised; pass Zoptimiser=false")
        AGP.likelihood(model) isa Union{AGP.LogisticLikelihood,AGP.StudentTLikelihood,AGP.LaplaceLikelihood} ||
            error("QuadratureVI on the HIP path runs for the Logistic, StudentT and Laplace likelihoods")
        AGP.inference(model).clipping == 0 || error("QuadratureVI: clipping != 0 is not offered (quadratureVI.jl:121-126)")
        all(gp -> AGP.opt(gp) === nothing, latents(model)) ||
            error("QuadratureVI: the hyper-parameter step through the quadrature ELBO is not built; pass optimiser=false")
    end
    return HipModel{T,M}(model, C_NULL, C_NULL, C_NULL, AGP_SHARD_LATENT, latent_range, 0, nothing, nothing, 0, nothing,
                         reference_compat_stale_K, Int32(0), Int32(1), Any[])
end

function ensure_ctx!(hm::HipModel)
    hm.ctx == C_NULL || return hm.ctx
    ctx = Ref{Ptr{Cvoid}}()
    stream = AMDGPU.stream().stream                          # share AMDGPU.jl's HIP stream with the library
    st = ccall((:agp_ctx_create, libagp), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), AMDGPU.device_id() - 1, stream, ctx)
    st == 0 || throw(AGPError(st, "agp_ctx_create"))
    hm.ctx = ctx[]
    finalizer(destroy!, hm)
    return hm.ctx
end

function destroy!(hm::HipModel)
    hm.h == C_NULL || ccall((:agp_svgp_destroy, libagp), Int32, (Ptr{Cvoid},), hm.h)
    hm.comm == C_NULL || ccall((:agp_comm_destroy, libagp), Int32, (Ptr{Cvoid},), hm.comm)
    hm.ctx == C_NULL || ccall((:agp_ctx_destroy, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    hm.h = hm.comm = hm.ctx = C_NULL
    return nothing
end

# (re)create the device handle for batches up to `maxbatch`; the posterior and the optimiser counters travel (get/set_state)
function ensure_handle!(hm::HipModel{T}, maxbatch::Int) where {T}
    (hm.h != C_NULL && maxbatch <= hm.maxbatch) && return hm.h
    ctx = ensure_ctx!(hm)
    model = hm.model
    old = hm.h == C_NULL ? nothing : (pull_posterior!(hm); opt_state(hm))
    hm.h == C_NULL || ccall((:agp_svgp_destroy, libagp), Int32, (Ptr{Cvoid},), hm.h)
    inf = AGP.inference(model)
    gp1 = latents(model)[first(hm.latent_range)]
    D = length(first(zview(hm, gp1)))
    m = AGP.dim(gp1)
    is_full(hm) && (maxbatch = m)                            # a VGP steps on its whole training set (idx = NULL, B = N = m)
    stoch = !is_sampled(hm) && AGP.is_stochastic(inf)
    rm = stoch ? inf.vi_opt.optimiser : nothing             # RobbinsMonro(κ, τ), optimisers.jl:1-19
    stoch && !(rm isa AGP.RobbinsMonro) && error("only RobbinsMonro is wired on this path (ALRSVI is dead code in the reference)")
    ld = is_mo(hm) ? LikDesc(4, 1, 0.0, 0.0) : lik_desc(AGP.likelihood(model))
    desc = SvgpDesc(T == Float64 ? 0 : 1, nlat(hm), first(hm.latent_range) - 1, stoch ? 1 : 0, m, D, maxbatch, ld, 0.0,
                    stoch ? rm.κ : 0.51, stoch ? rm.τ : 1.0, 0,
                    (hm.stale_K ? AGP_FLAG_STALE_K : Int32(0)) | (is_full(hm) ? AGP_FLAG_FULL : Int32(0)) |
                    (is_exact(hm) ? AGP_FLAG_EXACT : Int32(0)) | (is_sampled(hm) ? AGP_FLAG_SAMPLED : Int32(0)) |
                    (is_numerical(hm) ? AGP_FLAG_NUMERICAL : Int32(0)))
    h = Ref{Ptr{Cvoid}}()
    check(ctx, ccall((:agp_svgp_create, libagp), Int32, (Ptr{Cvoid}, Ref{SvgpDesc}, Ptr{Ptr{Cvoid}}), ctx, desc, h))
    hm.h, hm.maxbatch = h[], maxbatch
    for (i, q) in enumerate(hm.latent_range)
        gp = latents(model)[q]
        kd, keep = kernel_desc(AGP.kernel(gp), D)
        GC.@preserve keep check(ctx, ccall((:agp_svgp_set_kernel, libagp), Int32, (Ptr{Cvoid}, Int32, Ref{KernelDesc}), hm.h, i - 1, kd))
        Zd = ROCArray{T}(reduce(hcat, zview(hm, gp)))       # D x m, point-major
        check(ctx, ccall((:agp_svgp_set_Z, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64), hm.h, i - 1, pointer(Zd), D))
        μ₀ = AGP.pr_mean(gp)
        if !(μ₀ isa AGP.ZeroMean)   # (with an optimiser the FIRST HYPER STEP errors, like the reference's own broken update: update_hyperparameters!)
            v = ROCArray{T}(μ₀(zview(hm, gp)))
            check(ctx, ccall((:agp_svgp_set_prior_mean, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), hm.h, i - 1, pointer(v)))
        end
        AMDGPU.synchronize()
    end
    if is_mo(hm)
        liks = collect(AGP.likelihood(model))
        lds = [lik_desc(l) for l in liks]
        Q = length(latents(model))
        A = Matrix{Float64}(undef, length(liks), Q)          # model.A[t][j][q]; nf_per_task == 1 on this path
        for t in 1:length(liks), q in 1:Q
            A[t, q] = model.A[t][1][q]
        end
        Aopt = model.A_opt
        nlat(hm) == Q || check(ctx, ccall((:agp_svgp_mo_shard, libagp), Int32, (Ptr{Cvoid}, Int32), hm.h, Q))
        check(ctx, ccall((:agp_svgp_set_multioutput, libagp), Int32,
                         (Ptr{Cvoid}, Int32, Ptr{LikDesc}, Ptr{Float64}, Float64, Float64, Float64, Float64),
                         hm.h, length(liks), lds, permutedims(A), Aopt === nothing ? 0.0 : Aopt.eta, 0.9, 0.999, 1e-8))
    elseif AGP.likelihood(model) isa AGP.PoissonLikelihood    # the λ update integrates logistic by Gauss-Hermite (utils.jl:16-19)
        check(ctx, ccall((:agp_svgp_set_quadrature, libagp), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32),
                         hm.h, AGP.pred_nodes, AGP.pred_weights, length(AGP.pred_nodes)))
    end
    is_numerical(hm) && nvi_configure!(hm)
    # hyper-parameter optimisers: SVGP(...; optimiser, Zoptimiser) (SVGP.jl:39-42, default ADAM(0.01) / nothing)
    ko, zo = AGP.opt(gp1), is_full(hm) ? nothing : AGP.Zopt(gp1)   # (the inputs of a VGP are never optimised)
    is_sampled(hm) && (ko = nothing)                               # (the kernel of an MCGP is never tuned; the handle refuses the call)
    if ko !== nothing || zo !== nothing
        # the reference hands whatever Optimisers.jl rule it is given to Optimisers.apply (autotuning_utils.jl:47-82); the device
        # carries ADAM, Descent and Momentum (agp_svgp_hyper_rule), anything else is refused here rather than silently replaced
        rule(o) = o === nothing || o isa Optimisers.ADAM ? (0, 0.0) : o isa Optimisers.Descent ? (1, 0.0) :
                  o isa Optimisers.Momentum ? (2, Float64(o.rho)) :
                  error("hyper-parameter optimiser $(typeof(o)) is not available on the device (ADAM, Descent, Momentum are)")
        (kr, kρ), (zr, zρ) = rule(ko), rule(zo)
        adam = ko isa Optimisers.ADAM ? ko : zo isa Optimisers.ADAM ? zo : Optimisers.ADAM()
        check(ctx, ccall((:agp_svgp_hyper_configure, libagp), Int32,
                         (Ptr{Cvoid}, Int32, Float64, Int32, Float64, Float64, Float64, Float64),
                         hm.h, ko === nothing ? 0 : 1, ko === nothing ? 0.0 : ko.eta, zo === nothing ? 0 : 1,
                         zo === nothing ? 0.0 : zo.eta, adam.beta[1], adam.beta[2], 1e-8))
        check(ctx, ccall((:agp_svgp_hyper_rule, libagp), Int32, (Ptr{Cvoid}, Int32, Float64, Int32, Float64), hm.h, kr, kρ, zr, zρ))
    end
    if old !== nothing
        push_posterior!(hm)
        check(ctx, ccall((:agp_svgp_set_opt_state, libagp), Int32, (Ptr{Cvoid}, Int64), hm.h, old))
    end
    # a handle created (or re-created for a larger batch) AFTER comm_init! must know its shard too: the once-per-evaluation ELBO
    # terms and the Gaussian-KL weight of the hyper-gradient depend on it (the *_multi calls also take it from the communicator)
    if hm.comm != C_NULL && hm.shard == AGP_SHARD_BATCH
        check(ctx, ccall((:agp_svgp_set_batch_shard, libagp), Int32, (Ptr{Cvoid}, Int32, Int32), hm.h, hm.rank, hm.world))
    end
    return hm.h
end

opt_state(hm::HipModel) = (n = Ref{Int64}(); ccall((:agp_svgp_get_opt_state, libagp), Int32, (Ptr{Cvoid}, Ref{Int64}), hm.h, n); n[])

# (μ, Σ, η₁, η₂) device -> the reference's VarPosterior (posterior.jl:21-27), e.g. at the end of train!
function pull_posterior!(hm::HipModel{T}) where {T}
    is_exact(hm) && return pull_gp_posterior!(hm)
    is_numerical(hm) && return pull_nvi_posterior!(hm)
    for (i, q) in enumerate(hm.latent_range)
        gp = latents(hm.model)[q]
        m = AGP.dim(gp)
        μ = ROCVector{T}(undef, m); η₁ = ROCVector{T}(undef, m)
        Σ = ROCMatrix{T}(undef, m, m); η₂ = ROCMatrix{T}(undef, m, m)
        check(hm.ctx, ccall((:agp_svgp_get_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hm.h, i - 1, pointer(μ), pointer(Σ), pointer(η₁), pointer(η₂)))
        ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
        gp.post.μ .= Array(μ); gp.post.η₁ .= Array(η₁)
        gp.post.Σ.data .= Array(Σ); gp.post.η₂.data .= Array(η₂)   # symmetric: row-major == column-major
    end
    return hm
end
# the reference's (η₁, η₂) -> device (a model trained on the CPU continues on the GPU)
function push_posterior!(hm::HipModel{T}) where {T}
    for (i, q) in enumerate(hm.latent_range)
        gp = latents(hm.model)[q]
        η₁ = ROCArray{T}(AGP.nat1(gp)); η₂ = ROCArray{T}(Matrix(AGP.nat2(gp)))
        check(hm.ctx, ccall((:agp_svgp_set_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}), hm.h, i - 1, pointer(η₁), pointer(η₂)))
    end
    return hm
end

# kernel parameters / Z (device, after hyper steps) -> the reference objects; λ of Poisson / Heteroscedastic likewise
function pull_hypers!(hm::HipModel{T}) where {T}
    for (i, q) in enumerate(hm.latent_range)
        gp = latents(hm.model)[q]
        zopt = is_full(hm) ? nothing : AGP.Zopt(gp)          # (the inputs of a VGP / GP are never optimised)
        (AGP.opt(gp) === nothing && zopt === nothing) && continue
        D = length(first(zview(hm, gp))); m = AGP.dim(gp)
        σ² = Ref{Float64}(); sc = Vector{Float64}(undef, D)
        check(hm.ctx, ccall((:agp_svgp_get_kernel, libagp), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}, Ptr{Float64}), hm.h, i - 1, σ², sc))
        pull_kernel!(AGP.kernel(gp), σ²[], sc)
        is_full(hm) && continue
        Zd = ROCMatrix{T}(undef, D, m)
        check(hm.ctx, ccall((:agp_svgp_get_Z, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64), hm.h, i - 1, pointer(Zd), D))
        Zh = Array(Zd)
        for j in 1:m
            AGP.Zview(gp)[j] .= view(Zh, :, j)
        end
    end
    l = AGP.likelihood(hm.model)
    if l isa Union{AGP.PoissonLikelihood,AGP.HeteroscedasticGaussianLikelihood}
        v = Ref{Float64}()
        check(hm.ctx, ccall((:agp_svgp_get_lik_param, libagp), Int32, (Ptr{Cvoid}, Ref{Float64}), hm.h, v))
        l.invlink.λ .= v[]                                   # poisson.jl:78, heteroscedastic.jl:95 mutate it in place
    end
    if l isa GaussianLikelihood && l.opt_noise !== nothing   # gaussian.jl:69 mutates l.σ² in place
        v = Ref{Float64}()
        check(hm.ctx, ccall((:agp_svgp_get_lik_param, libagp), Int32, (Ptr{Cvoid}, Ref{Float64}), hm.h, v))
        l.σ² .= v[]
    end
    if is_mo(hm)
        liks = AGP.likelihood(hm.model); Q = length(latents(hm.model))
        A = Matrix{Float64}(undef, Q, length(liks))          # row-major n_task x Q on the C side
        check(hm.ctx, ccall((:agp_svgp_get_A, libagp), Int32, (Ptr{Cvoid}, Ptr{Float64}), hm.h, A))
        for t in 1:length(liks), q in 1:Q
            hm.model.A[t][1][q] = A[q, t]
        end
    end
    return hm
end

# ---- data ---------------------------------------------------------------------------------------------------------------------
# wrap_X / wrap_data (src/data/datacontainer.jl:18-74, src/data/utils.jl:16-30): labels are normalised by the reference's own
# treat_labels!, then laid out for the device: ±1 / real T[N]; class index Int32[N] (0-based row-wise findfirst of the one-hot
# BitMatrix, multiclass.jl:81-94); multi-output T[n_task x N] (point-major)
function upload!(hm::HipModel{T}, X::AbstractMatrix, y; obsdim::Int=1) where {T}
    Xv, _ = AGP.wrap_X(X, obsdim)
    data = AGP.wrap_data(Xv, y, AGP.likelihood(hm.model))     # runs treat_labels! (ArgumentErrors surface here)
    yt = AGP.output(data)
    hm.X = ROCArray{T}(obsdim == 1 ? permutedims(X) : X)      # one-time RowVecs -> point-major permutation
    hm.N = size(hm.X, 2)
    if is_mo(hm)
        hm.y = ROCArray{T}(permutedims(reduce(hcat, yt)))     # n_task x N
    elseif is_multiclass(AGP.likelihood(hm.model))
        hm.y = ROCArray(Int32.(map(r -> findfirst(r) - 1, eachrow(yt))))
    else
        hm.y = ROCArray{T}(yt)
    end
    return data
end

# ---- update_parameters!(model, state, x, y) (training.jl:140-158) ---------------------------------------------------------------
# `idx` is the minibatch drawn by train! (StatsBase.sample, training.jl:51-53), 1-based; nothing = full batch.
# minibatch indices on the device, 0-based (an already uploaded vector is taken as it is: the look-ahead and the step that
# consumes it must see the same buffer)
device_indices(idx::Nothing) = nothing
device_indices(idx::ROCArray{Int64}) = idx
device_indices(idx::AbstractVector{<:Integer}) = ROCArray(Int64.(idx .- 1))

function update_parameters!(hm::HipModel{T}, idx, ρ::Real) where {T}
    D = size(hm.X, 1)
    idd = device_indices(idx)
    hm.last_idx = idd
    B = idx === nothing ? hm.N : length(idx)
    idp = idd === nothing ? Ptr{Int64}(C_NULL) : pointer(idd)
    st = if is_numerical(hm)   # variational_updates of numericalVI.jl:101-119 (the whole training set: idx = NULL, rho = 1)
        ccall((:agp_svgp_nvi_step, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64),
              hm.h, pointer(hm.X), D, pointer(hm.y), idp, B, ρ)
    elseif hm.comm == C_NULL && nlat(hm) == length(latents(hm.model))
        ccall((:agp_svgp_cavi_step, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64),
              hm.h, pointer(hm.X), D, pointer(hm.y), idp, B, ρ)
    else
        ccall((:agp_svgp_cavi_step_multi, libagp), Int32,
              (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64),
              hm.h, hm.comm, hm.shard, pointer(hm.X), D, pointer(hm.y), idp, B, ρ)
    end
    check(hm.ctx, st)
    return nothing
end

# Look-ahead: Knm / kappa of the NEXT minibatch on the library's second stream, next to the current step's factorisation
# (agp_svgp_prefetch; a no-op while K is stale, i.e. right after a hyper-parameter step).  `idd` must be the very buffer the next
# update_parameters! passes.
function prefetch!(hm::HipModel, idd::ROCArray{Int64})
    D = size(hm.X, 1)
    check(hm.ctx, ccall((:agp_svgp_prefetch, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Int64),
                        hm.h, pointer(hm.X), D, pointer(idd), length(idd)))
    return nothing
end

# update_hyperparameters!(m, state, x, y) (autotuning.jl:86-140) on the minibatch of the last step
function update_hyperparameters!(hm::HipModel; tied::Bool=false)
    # (a GP's prior mean is never stepped: its update_hyperparameters! has no prior-mean part, autotuning.jl:5-37)
    !is_exact(hm) && any(gp -> !(AGP.pr_mean(gp) isa AGP.ZeroMean), latents(hm.model)[hm.latent_range]) &&
        error("a non-zero prior mean with hyper-parameter optimisation is not wired: the reference's own prior-mean update " *
              "(autotuning.jl:104-106 vs src/mean/constantmean.jl:31) cannot run")
    st = hm.comm == C_NULL && !tied ? ccall((:agp_svgp_hyper_step, libagp), Int32, (Ptr{Cvoid},), hm.h) :
         ccall((:agp_svgp_hyper_step_multi, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), hm.h, hm.comm, tied ? 1 : 0)
    check(hm.ctx, st)
end

"""
    hyper_counters(hm) -> (gradients, gradients_with_one_product_G_K)

Diagnostics of the hyper-parameter iteration (`agp_svgp_hyper_counters`, round 4): how many hyper-gradients this handle has
evaluated, and how many of them formed `G_K` from one m^3 product (DESIGN.md section 6) instead of `kappa' H` and `K^-1 Sigma K^-1`.
"""
function hyper_counters(hm::HipModel)
    ng = Ref{Int64}(0); nf = Ref{Int64}(0)
    check(hm.ctx, ccall((:agp_svgp_hyper_counters, libagp), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), hm.h, ng, nf))
    return ng[], nf[]
end

"""
    train!(hm::HipModel, X, y, iterations=100; callback=nothing, state=nothing, obsdim=1, idx_stream=nothing)

`train!` of the reference (src/training/training.jl:13-111) with the step on the device: same checks, same ρ = N/B, same
`StatsBase.sample(1:N, B; replace=false)` per iteration (or the caller's `idx_stream`, one index vector per iteration, so that
runs are reproducible across back-ends), same hyper-step gating (`n_iter % atfrequency == 0 && n_iter >= 3 &&
local_iter != iterations`, :65-69), fixed iteration count (the reference never reads `convergence` / ϵ, :48,93-94), final
`compute_Ks` (:107).  Returns `(hm, state)`; the state is the device-resident one: pass it back (`state=state`) to continue, or
omit it to restart counters and local variables like the reference's `init_state` (states.jl:1-9).
"""
function train!(hm::HipModel{T}, X::AbstractArray, y, iterations::Int=100; callback=nothing, convergence=nothing,
                state=nothing, obsdim=1, idx_stream=nothing) where {T}
    iterations > 0 || error("Number of iterations should be positive")
    model = hm.model
    inf = AGP.inference(model)
    data = upload!(hm, X isa AbstractMatrix ? X : reduce(hcat, X)', y; obsdim)
    N = hm.N
    if AGP.is_stochastic(model)
        0 < AGP.batchsize(inf) <= N || error(
            "The size of mini-batch $(AGP.batchsize(inf)) is incorrect (negative or bigger than number of samples), please set `batchsize` correctly in the inference object")
        AGP.set_ρ!(model, N / AGP.batchsize(inf))
    else
        AGP.set_batchsize!(inf, N)
    end
    B = AGP.batchsize(inf)
    Blocal = (hm.comm != C_NULL && hm.shard == AGP_SHARD_BATCH) ? B ÷ comm_world(hm) : B
    ensure_handle!(hm, Blocal)
    if state === nothing
        AGP.setHPupdated!(inf, true)
        check(hm.ctx, ccall((:agp_svgp_init_state, libagp), Int32, (Ptr{Cvoid},), hm.h))      # init_state(model), training.jl:41-45
    else
        check(hm.ctx, ccall((:agp_svgp_invalidate_data, libagp), Int32, (Ptr{Cvoid},), hm.h)) # the buffers were re-uploaded
    end
    check(hm.ctx, ccall((:agp_svgp_refresh_K, libagp), Int32, (Ptr{Cvoid},), hm.h))
    ρ = AGP.is_stochastic(model) ? N / B : 1.0
    hyper_on = any(gp -> AGP.opt(gp) !== nothing || (!is_full(hm) && AGP.Zopt(gp) !== nothing), latents(model))
    # minibatch of iteration `it` on the device: the reference's sample(1:N, B; replace=false) (training.jl:51-53), drawn in the
    # same order, one iteration ahead of its use so that the look-ahead can run next to the current step
    function draw(it)
        AGP.is_stochastic(model) || return nothing
        idx = idx_stream === nothing ? sample(1:N, B; replace=false) : idx_stream[it]
        if hm.comm != C_NULL && hm.shard == AGP_SHARD_BATCH    # this rank's share of the minibatch (rho stays N / B_total)
            r = comm_rank(hm)
            idx = idx[(r * Blocal + 1):((r + 1) * Blocal)]
        end
        return device_indices(idx)
    end
    if AGP.verbose(model) > 0   # training.jl:35-38
        @info "Starting training $model with $N samples, $(size(hm.Xd, 1)) features and $(length(latents(model))) latent GP" *
              (length(latents(model)) > 1 ? "s" : "")
    end
    local_iter = 1
    # progress reporting of the reference (training.jl:46,71-90): ProgressMeter with (:iter, :ELBO); the ELBO is
    # `objective(model, state, y)` on the kernel matrices / local variables of the step just taken -- verbose == 2: every 10th
    # iteration, verbose > 2: every iteration.  On the device the value is ENQUEUED behind the step (agp_svgp_elbo_enqueue) and shown
    # one report later, so that reporting never makes the host wait for the stream inside the loop.
    prog = AGP.verbose(model) > 1 ? ProgressMeter.Progress(iterations; dt=0.2, desc="Training Progress: ") : nothing
    pending_elbo = nothing   # (ticket, iteration it belongs to)
    function report(it)
        prog === nothing && return
        (AGP.verbose(model) > 2 || it % 10 == 0) || return
        if is_exact(hm)   # log p of a GP is read synchronously: an exact handle refuses agp_svgp_elbo_enqueue
            AGP.verbose(model) == 2 && ProgressMeter.update!(prog, it - 1)
            ProgressMeter.next!(prog; showvalues=[(:iter, it), (:ELBO, objective(hm))])
            return
        end
        tk = objective_enqueue(hm)
        if pending_elbo !== nothing
            elbo = objective_fetch(hm, pending_elbo[1])
            AGP.verbose(model) == 2 && ProgressMeter.update!(prog, pending_elbo[2] - 1)
            ProgressMeter.next!(prog; showvalues=[(:iter, pending_elbo[2]), (:ELBO, elbo)])
        end
        pending_elbo = (tk, it)
    end
    idd = draw(1)
    while true
        stepped = false   # this iteration's variational update has been enqueued (the device's own counters have moved on)
        try
        update_parameters!(hm, idd, ρ)
        stepped = true
        AGP.set_trained!(model, true)
        # the next minibatch is drawn now and its look-ahead enqueued right behind the step (next to its factorisation) -- unless a
        # hyper step follows: it moves the kernel / Z, a look-ahead against the old ones would be thrown away (agp_svgp_prefetch
        # contract, include/agp_hip.h; the Python mirror skips it the same way, svgp.py train_)
        hyper_now = hyper_on && (AGP.n_iter(model) % model.atfrequency == 0) && (AGP.n_iter(model) >= 3) && (local_iter != iterations)
        nxt = local_iter < iterations ? draw(local_iter + 1) : nothing
        # index buffers stay referenced for two iterations: the look-ahead reads `nxt`, and the step's natural-gradient part is
        # taken by the NEXT launch (it reads device copies only, but the buffer identity is what the look-ahead is recognised by)
        push!(hm.keep, idd); length(hm.keep) > 3 && popfirst!(hm.keep)
        (nxt === nothing || hyper_now || is_numerical(hm)) || prefetch!(hm, nxt)   # (a numerical handle has no look-ahead)
        callback === nothing || callback(hm, hm, AGP.n_iter(model))
        hyper_now && update_hyperparameters!(hm)
        report(local_iter)
        local_iter += 1
        inf.n_iter += 1
        (local_iter <= iterations) || break
        idd = nxt
        catch e
            # training.jl:95-101: an InterruptException ends the loop with a warning, everything else is rethrown.  A variational
            # update that was already enqueued counts (its Robbins-Monro step has been taken on the device); the pending natural-
            # gradient step is taken by agp_svgp_check_status below, and `state=` continues from there.
            if isa(e, InterruptException)
                @warn "Training interrupted by user at iteration $local_iter"
                if stepped
                    local_iter += 1
                    inf.n_iter += 1
                end
                break
            else
                rethrow(e)
            end
        end
    end
    pending_elbo === nothing || objective_fetch(hm, pending_elbo[1])   # (close the last report's ticket)
    if AGP.verbose(model) > 0   # training.jl:103-105
        @info "Training ended after $(local_iter - 1) iterations. Total number of iterations $(AGP.n_iter(model))"
    end
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    check(hm.ctx, ccall((:agp_svgp_refresh_K, libagp), Int32, (Ptr{Cvoid},), hm.h))            # compute_Ks, training.jl:107
    pull_posterior!(hm)                                       # the reference object is usable on the CPU again
    pull_hypers!(hm)
    AGP.set_trained!(model, true)
    return hm, hm
end

# ---- ELBO ------------------------------------------------------------------------------------------------------------------------
# objective(model, state, y) = ELBO(model, state, y) on the last minibatch (SVGP.jl:90, analyticVI.jl:255-297)
function objective(hm::HipModel, state=nothing, y=nothing)
    out = Ref{Float64}()
    if hm.comm != C_NULL
        check(hm.ctx, ccall((:agp_svgp_elbo_multi, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Float64}), hm.h, hm.comm, hm.shard, out))
        return out[]
    end
    B = hm.last_idx === nothing ? hm.N : length(hm.last_idx)
    ρ = AGP.is_stochastic(hm.model) ? hm.N / B : 1.0
    idp = hm.last_idx === nothing ? Ptr{Int64}(C_NULL) : pointer(hm.last_idx)
    check(hm.ctx, ccall((:agp_svgp_elbo, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64, Int32, Ref{Float64}),
                        hm.h, pointer(hm.X), size(hm.X, 1), pointer(hm.y), idp, B, ρ, 0, out))
    return out[]
end

# the same evaluation put into the stream without waiting for it (agp_svgp_elbo_enqueue / agp_svgp_elbo_fetch): a callback that
# monitors convergence enqueues `t = objective_enqueue(hm)` and reads `objective_fetch(hm, t)` an iteration or ten later, so the
# training loop never synchronises with the device (up to 8 tickets in flight)
function objective_enqueue(hm::HipModel)
    B = hm.last_idx === nothing ? hm.N : length(hm.last_idx)
    ρ = AGP.is_stochastic(hm.model) ? hm.N / B : 1.0
    idp = hm.last_idx === nothing ? Ptr{Int64}(C_NULL) : pointer(hm.last_idx)
    t = Ref{Int32}()
    check(hm.ctx, ccall((:agp_svgp_elbo_enqueue, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64, Int32, Ref{Int32}),
                        hm.h, pointer(hm.X), size(hm.X, 1), pointer(hm.y), idp, B, ρ, 0, t))
    return t[]
end
function objective_fetch(hm::HipModel, ticket::Integer; wait::Bool=true)
    out, ready = Ref{Float64}(), Ref{Int32}()
    check(hm.ctx, ccall((:agp_svgp_elbo_fetch, libagp), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Float64}, Ref{Int32}),
                        hm.h, ticket, wait ? 1 : 0, out, ready))
    return ready[] == 1 ? out[] : nothing
end

"""
    task_graph_fallbacks(hm) -> Int

How many factorisation launches of this model's context lost a tile dependency and were re-run by their in-stream fallback since the
context was created (`agp_ctx_task_graph_fallbacks`, round 6): 0 on a GPU the process has to itself.  Synchronises the stream.
"""
function task_graph_fallbacks(hm::HipModel)
    n = Ref{Int64}(0)
    check(hm.ctx, ccall((:agp_ctx_task_graph_fallbacks, libagp), Int32, (Ptr{Cvoid}, Ref{Int64}), hm.ctx, n))
    return Int(n[])
end

"""
    SideObjective(hm::HipModel, max_eval_batch; ring=4)
    ticket = enqueue!(side, idx::ROCVector{Int64}, ρ)     # snapshot of (η₁, η₂) now, ELBO(model, X[idx], y[idx]) on the side stream
    value  = fetch(side, ticket; wait=true)

Convergence monitoring NEXT TO the training stream (round 6; the Python mirror's `agp_amd.SideObjective`, same three ABI calls): a
shadow `HipModel` of a deep copy of the reference model on a HIP stream and context of its own, its K_ZZ factored once; `enqueue!`
copies (η₁, η₂) out of the training handle on the training stream (`agp_svgp_get_state`, two device copies), makes the side stream wait
for them (`AMDGPU.HIP` event), installs them there (`agp_svgp_set_state`) and enqueues the evaluation (`agp_svgp_elbo_enqueue`, fresh
local variables: `ELBO(model, X, y)` of src/functions/ELBO.jl:32-47 with ρ explicit).  Replaces the in-line `objective(model, state, y)`
of `train!`'s progress reporting (src/training/training.jl:71-90) where the host must not wait and the training stream must not carry
the evaluation.  Kernels and inducing points must be fixed (`optimiser=false, Zoptimiser=false`): the shadow's K_ZZ is factored once.
The values equal the in-line evaluation's to a few ulp; the training trajectory with snapshots equals the one without to rounding.
"""
mutable struct SideObjective{T}
    hm::HipModel{T}
    shadow::HipModel{T}
    stream::AMDGPU.HIPStream
    ring::Vector{Tuple{ROCVector{T},ROCMatrix{T},AMDGPU.HIP.HIPEvent,AMDGPU.HIP.HIPEvent}}
    n::Int
end

function SideObjective(hm::HipModel{T}, max_eval_batch::Int; ring::Int=4) where {T}
    (length(latents(hm.model)) == 1 && !is_mo(hm) && !is_exact(hm)) || error("SideObjective: single-latent SVGP models")
    all(gp -> AGP.opt(gp) === nothing && AGP.Zopt(gp) === nothing, latents(hm.model)) ||
        error("SideObjective: kernels and inducing points must be fixed (optimiser=false, Zoptimiser=false)")
    hm.h != C_NULL || error("SideObjective: the model has no device state yet")
    stream = AMDGPU.HIPStream()
    shadow = HipModel(deepcopy(hm.model))
    AMDGPU.stream!(stream) do                                  # the shadow's context takes AMDGPU.jl's current stream: the side stream
        shadow.X, shadow.y, shadow.N = hm.X, hm.y, hm.N        # (the same device data: read-only on both sides)
        ensure_handle!(shadow, max_eval_batch)
        check(shadow.ctx, ccall((:agp_svgp_refresh_K, libagp), Int32, (Ptr{Cvoid},), shadow.h))
    end
    AMDGPU.synchronize(stream)
    m = AGP.dim(latents(hm.model)[1])
    slots = [(ROCVector{T}(undef, m), ROCMatrix{T}(undef, m, m), AMDGPU.HIP.HIPEvent(stream), AMDGPU.HIP.HIPEvent(stream)) for _ in 1:ring]
    return SideObjective{T}(hm, shadow, stream, slots, 0)
end

function enqueue!(side::SideObjective{T}, idx::ROCVector{Int64}, ρ::Real) where {T}
    hm, sh = side.hm, side.shadow
    e1, e2, ev_snap, ev_used = side.ring[side.n % length(side.ring) + 1]
    main = AMDGPU.stream()
    side.n >= length(side.ring) && AMDGPU.HIP.wait(ev_used, main)   # the side stream has installed what this slot held
    check(hm.ctx, ccall((:agp_svgp_get_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, 0, C_NULL, C_NULL, pointer(e1), pointer(e2)))
    AMDGPU.HIP.record(ev_snap, main)
    tk = Ref{Int32}()
    AMDGPU.stream!(side.stream) do
        AMDGPU.HIP.wait(ev_snap, side.stream)
        check(sh.ctx, ccall((:agp_svgp_set_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}), sh.h, 0, pointer(e1), pointer(e2)))
        AMDGPU.HIP.record(ev_used, side.stream)
        check(sh.ctx, ccall((:agp_svgp_elbo_enqueue, libagp), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64, Int32, Ref{Int32}),
                            sh.h, pointer(hm.X), size(hm.X, 1), pointer(hm.y), pointer(idx), length(idx), Float64(ρ), 1, tk))
    end
    side.n += 1
    return tk[]
end

Base.fetch(side::SideObjective, ticket::Integer; wait::Bool=true) = objective_fetch(side.shadow, ticket; wait)

# external ELBO(model, X, y) (src/functions/ELBO.jl:28-47): kernel matrices recomputed on (X, y), fresh local variables, one local
# update.  The reference keeps ρ = N/B of the last train! here (Appendix A Q13); pass ρ = 1 for the properly scaled value.
# streamed=true: the same value over ANY number of points (agp_svgp_elbo_stream): chunks of 4096 through the predictor's kernels,
# the handle is not re-created with max_batch = n, the workspace does not depend on n.  Sparse AnalyticVI / AnalyticSVI models;
# the library refuses the others by name (include/agp_hip.h, "STREAMED ELBO").
function ELBO(hm::HipModel{T}, X::AbstractMatrix, y::AbstractArray; obsdim=1, ρ::Real=AGP.ρ(AGP.inference(hm.model)),
              streamed::Bool=false) where {T}
    twin = HipModel{T,typeof(hm.model)}(hm.model, hm.ctx, hm.h, C_NULL, hm.shard, hm.latent_range, hm.maxbatch, nothing, nothing,
                                        0, nothing, hm.stale_K, hm.rank, hm.world, Any[])  # same handle, its own data buffers
    upload!(twin, X, y; obsdim)
    n = twin.N
    if streamed
        ensure_handle!(hm, max(hm.maxbatch, 1))
        out = Ref{Float64}()
        check(hm.ctx, ccall((:agp_svgp_elbo_stream, libagp), Int32,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64, Ref{Float64}, Ptr{Float64}),
                            hm.h, pointer(twin.X), size(twin.X, 1), pointer(twin.y), C_NULL, n, ρ, out, C_NULL))
        return out[]
    end
    if n > hm.maxbatch
        ensure_handle!(hm, n); twin.h = hm.h
    end
    out = Ref{Float64}()
    check(hm.ctx, ccall((:agp_svgp_elbo, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Float64, Int32, Ref{Float64}),
                        hm.h, pointer(twin.X), size(twin.X, 1), pointer(twin.y), C_NULL, n, ρ, 1, out))
    return out[]
end

# ---- prediction (src/training/predictions.jl) --------------------------------------------------------------------------------------
function _predict_f_dev(hm::HipModel{T}, Xt::AbstractMatrix; cov::Bool, obsdim::Int=1) where {T}
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(Xt) : Xt)
    D, nt = size(Xd)
    nout = is_mo(hm) ? length(AGP.likelihood(hm.model)) : nlat(hm)
    μ = ROCMatrix{T}(undef, nt, nout)                        # column l == latent / task l  (ABI: T[n_out][n_t])
    v = cov ? ROCMatrix{T}(undef, nt, nout) : nothing
    check(hm.ctx, ccall((:agp_svgp_predict_f, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, pointer(Xd), D, nt, pointer(μ), cov ? pointer(v) : C_NULL))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    return Array(μ), (cov ? Array(v) : nothing), Xd
end

# predict_f(model, X_test; cov=false, diag=true) predictions.jl:141-164: Vector (one latent) or Tuple of Vectors
function predict_f(hm::HipModel{T}, X_test::AbstractMatrix, state=nothing; cov::Bool=false, diag::Bool=true, obsdim::Int=1) where {T}
    if cov && !diag                                           # full covariance, predictions.jl:45-49 (K*m materialised: small n_t)
        Xd = ROCArray{T}(obsdim == 1 ? permutedims(X_test) : X_test)
        D, nt = size(Xd); L = nlat(hm)
        μ = ROCMatrix{T}(undef, nt, L); Σ = ROCArray{T}(undef, nt, nt, L)
        check(hm.ctx, ccall((:agp_svgp_predict_f_cov, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                            ensure_handle!(hm, max(hm.maxbatch, 1)), pointer(Xd), D, nt, pointer(μ), pointer(Σ)))
        ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
        μh, Σh = Array(μ), Array(Σ)
        return L == 1 ? (μh[:, 1], Symmetric(Σh[:, :, 1])) : (Tuple(μh[:, l] for l in 1:L), Tuple(Symmetric(Σh[:, :, l]) for l in 1:L))
    end
    μ, v, _ = _predict_f_dev(hm, X_test; cov, obsdim)
    n = size(μ, 2)
    if n == 1 && !is_mo(hm)
        return cov ? (μ[:, 1], v[:, 1]) : μ[:, 1]
    end
    μt = Tuple(μ[:, l] for l in 1:n)
    return cov ? (μt, Tuple(v[:, l] for l in 1:n)) : μt
end

# ---- input gradients of the predictive moments (include/agp_hip.h, "PREDICTIVE GRADIENTS"; no counterpart in the reference) -----------
# predict_f_grad(hm, X_test; cov=true): (dμ, dσ²), n_t x D matrices with dμ[i, d] = ∂μ(x_i)/∂x_id of what predict_f returns (dμ alone
# with cov=false); Tuples over the latents / tasks where predict_f returns Tuples.  SqExponential / Matern32 / Matern52 kernels,
# D <= 64; the library refuses Gibbs-sampled and sharded handles, the ExponentialKernel and D > 64 by name.
function predict_f_grad(hm::HipModel{T}, X_test::AbstractMatrix; cov::Bool=true, obsdim::Int=1) where {T}
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(X_test) : X_test)
    D, nt = size(Xd)
    nout = is_mo(hm) ? length(AGP.likelihood(hm.model)) : nlat(hm)
    gm = ROCArray{T}(undef, D, nt, nout)                     # column-major D x n_t x n_out == the ABI's T[n_out][n_t][ldg = D]
    gv = cov ? ROCArray{T}(undef, D, nt, nout) : nothing
    check(hm.ctx, ccall((:agp_svgp_predict_f_grad, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                        hm.h, pointer(Xd), D, nt, pointer(gm), cov ? pointer(gv) : C_NULL, D))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    gmh = Array(gm)
    gvh = cov ? Array(gv) : nothing
    if nout == 1 && !is_mo(hm)
        return cov ? (permutedims(gmh[:, :, 1]), permutedims(gvh[:, :, 1])) : permutedims(gmh[:, :, 1])
    end
    mt = Tuple(permutedims(gmh[:, :, l]) for l in 1:nout)
    return cov ? (mt, Tuple(permutedims(gvh[:, :, l]) for l in 1:nout)) : mt
end

# predict_y predictions.jl:178-198: regression mean / Bool / most likely class label / expected count
function predict_y(hm::HipModel{T}, X_test::AbstractMatrix, state=nothing; obsdim::Int=1) where {T}
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(X_test) : X_test)
    D, nt = size(Xd)
    l = AGP.likelihood(hm.model)
    if is_mo(hm)
        out = ROCMatrix{T}(undef, nt, length(l))
        check(hm.ctx, ccall((:agp_svgp_predict_y, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}), hm.h, pointer(Xd), D, nt, pointer(out)))
        o = Array(out)
        return [is_bernoulli(lt) ? o[:, t] .> 0.5 : o[:, t] for (t, lt) in enumerate(l)]
    elseif is_bernoulli(l) || is_multiclass(l)
        out = ROCVector{Int32}(undef, nt)
        check(hm.ctx, ccall((:agp_svgp_predict_y, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}), hm.h, pointer(Xd), D, nt, pointer(out)))
        o = Array(out)
        return is_bernoulli(l) ? o .== 1 : [l.class_mapping[i + 1] for i in o]     # multiclass.jl:96-99 / predictions.jl:200-202
    else
        out = ROCVector{T}(undef, nt)
        check(hm.ctx, ccall((:agp_svgp_predict_y, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}), hm.h, pointer(Xd), D, nt, pointer(out)))
        return Array(out)
    end
end

# proba_y predictions.jl:225-247 + compute_proba: (mean, var) for regression, p for Bernoulli, per-class probabilities
function proba_y(hm::HipModel{T}, X_test::AbstractMatrix, state=nothing; obsdim::Int=1) where {T}
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(X_test) : X_test)
    D, nt = size(Xd)
    l = AGP.likelihood(hm.model)
    nout = is_mo(hm) ? length(l) : 1
    o0 = is_multiclass(l) ? ROCMatrix{T}(undef, nlat(hm), nt) : ROCMatrix{T}(undef, nt, nout)
    o1 = is_multiclass(l) ? nothing : ROCMatrix{T}(undef, nt, nout)
    check(hm.ctx, ccall((:agp_svgp_proba_y, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, pointer(Xd), D, nt, AGP.pred_nodes, AGP.pred_weights, length(AGP.pred_nodes), pointer(o0),
                        o1 === nothing ? C_NULL : pointer(o1)))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    if is_multiclass(l)
        p = Array(o0)                                        # K x n_t (ABI: T[n_t][K] row-major)
        return NamedTuple{Tuple(Symbol.(l.class_mapping))}(Tuple(p[k, :] for k in 1:size(p, 1)))   # multiclass.jl:101-117
    end
    a, b = Array(o0), Array(o1)
    is_mo(hm) && return [(a[:, t], b[:, t]) for t in 1:nout]
    return is_bernoulli(l) ? a[:, 1] : (a[:, 1], b[:, 1])
end

# ---- log predictive density (include/agp_hip.h, "LOG PREDICTIVE DENSITY") ---------------------------------------------------------
# sum_i log p(y_i | x_i, model) over ANY number of test points (the held-out log-likelihood; its negative mean is the NLPD), streamed
# in chunks of 4096 through the handle's own predictor (agp_svgp_lpd_stream).  Gaussian and Laplace in closed form; Logistic,
# BayesianSVM, StudentT (the reference's density as written, studentt.jl:43-46), Poisson and NegBinomial by the Gauss-Hermite rule of
# predictions.jl:4 formed as a log-sum-exp; LogisticSoftMax by the link on the means (multiclass.jl:96-117).  Labels go through the
# reference's own treat_labels! (upload!).  pointwise=true: (sum, lpd::Vector).  The library refuses Heteroscedastic, multi-output,
# Gibbs-sampled and sharded handles by name.
function log_predictive_density(hm::HipModel{T}, X::AbstractMatrix, y::AbstractArray; pointwise::Bool=false, obsdim::Int=1,
                                nodes::Vector{Float64}=AGP.pred_nodes, weights::Vector{Float64}=AGP.pred_weights) where {T}
    twin = HipModel{T,typeof(hm.model)}(hm.model, hm.ctx, hm.h, C_NULL, hm.shard, hm.latent_range, hm.maxbatch, nothing, nothing,
                                        0, nothing, hm.stale_K, hm.rank, hm.world, Any[])  # same handle, its own data buffers
    upload!(twin, X, y; obsdim)
    n = twin.N
    ensure_handle!(hm, max(hm.maxbatch, 1))
    out = Ref{Float64}(0.0)
    vec = pointwise ? ROCVector{T}(undef, n) : nothing
    check(hm.ctx, ccall((:agp_svgp_lpd_stream, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ref{Float64}, Ptr{Cvoid}),
                        hm.h, pointer(twin.X), size(twin.X, 1), pointer(twin.y), n, nodes, weights, length(nodes), out,
                        vec === nothing ? C_NULL : pointer(vec)))
    return pointwise ? (out[], Array(vec)) : out[]
end

# the point-wise kernel on given moments, outside any model (agp_log_predictive): lpd[i] from y[i], mu[i], var[i]; for a multi-class
# likelihood y holds 0-based class indices (Int32) and mu, var are n x K.  The nodes are not needed for Gaussian, Laplace and the
# multi-class likelihoods.
function log_predictive_moments(l, y::AbstractVector, mu::AbstractVecOrMat{T}, var::AbstractVecOrMat{T};
                                nodes::Vector{Float64}=AGP.pred_nodes, weights::Vector{Float64}=AGP.pred_weights) where {T<:Union{Float32,Float64}}
    n = length(y)
    size(mu, 1) == n && size(mu) == size(var) || throw(DimensionMismatch("y has $n entries, mu and var must have n rows"))
    yd = is_multiclass(l) ? ROCVector{Int32}(y) : ROCVector{T}(y)
    md, vd = ROCArray{T}(mu), ROCArray{T}(var)                  # column-major n x K == T[K][n], latent stride n
    out = ROCVector{T}(undef, n)
    ctx = Ref{Ptr{Cvoid}}()
    st = ccall((:agp_ctx_create, libagp), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), AMDGPU.device_id() - 1, AMDGPU.stream().stream, ctx)
    st == 0 || throw(AGPError(st, "agp_ctx_create"))
    try
        check(ctx[], ccall((:agp_log_predictive, libagp), Int32,
                           (Ptr{Cvoid}, Int32, Ref{LikDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64},
                            Int32, Ptr{Cvoid}),
                           ctx[], T == Float64 ? Int32(0) : Int32(1), lik_desc(l), pointer(yd), pointer(md), pointer(vd), n, n, nodes,
                           weights, length(nodes), pointer(out)))
        return Array(out)
    finally
        ccall((:agp_ctx_destroy, libagp), Int32, (Ptr{Cvoid},), ctx[])
    end
end

# ---- multi-GPU: one Julia process per GPU ---------------------------------------------------------------------------------------
# rank 0:  id = AGPHip.comm_unique_id()  -> broadcast the 128 bytes (MPI.Bcast!, Distributed, a file ...)
# all:     AGPHip.comm_init!(hm, rank, world, id; shard=:batch | :latent)
# then train! / objective / update_hyperparameters! route through the *_multi entry points; RCCL runs on the model's stream.
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    st = ccall((:agp_comm_unique_id, libagp), Int32, (Ptr{UInt8},), id)
    st == 0 || throw(AGPError(st, "agp_comm_unique_id (librccl not found? set AGP_RCCL_PATH)"))
    return id
end
function comm_init!(hm::HipModel, rank::Integer, world::Integer, id::Vector{UInt8}; shard::Symbol=:batch)
    length(id) == 128 || throw(ArgumentError("the RCCL id has 128 bytes"))
    c = Ref{Ptr{Cvoid}}()
    check(ensure_ctx!(hm), ccall((:agp_comm_init, libagp), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ptr{Ptr{Cvoid}}),
                                 hm.ctx, rank, world, id, c))
    hm.comm = c[]
    hm.shard = shard === :batch ? AGP_SHARD_BATCH : AGP_SHARD_LATENT
    hm.rank, hm.world = Int32(rank), Int32(world)            # ensure_handle! re-applies them to every handle it creates later
    if shard === :batch && hm.h != C_NULL
        check(hm.ctx, ccall((:agp_svgp_set_batch_shard, libagp), Int32, (Ptr{Cvoid}, Int32, Int32), hm.h, rank, world))
    end
    return hm
end
function comm_info(hm::HipModel)
    r, w, k = Ref{Int32}(), Ref{Int32}(), Ref{Int32}()
    ccall((:agp_comm_info, libagp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), hm.comm, r, w, k)
    return Int(r[]), Int(w[]), k[] == 1
end
comm_rank(hm::HipModel) = comm_info(hm)[1]
comm_world(hm::HipModel) = comm_info(hm)[2]
# latent-parallel: build every rank's twin with HipModel(model; latent_range = latent_slice(length(model.f), world, rank))
function latent_slice(n::Int, world::Int, rank::Int)
    base, rem = divrem(n, world)
    lo = rank * base + min(rank, rem)
    return (lo + 1):(lo + base + (rank < rem ? 1 : 0))
end

# ---- inducing-point selection on the device (InducingPoints.jl's interface, agp_kmeans behind it) --------------------------------
# `inducingpoints(KmeansAlg(m), X)` is how every example / test of the reference picks Z (test/testingtools.jl:66,
# docs/examples/gpclassification.jl:47).  The random part (AFK-MC² seeding: first centre, proposals, Metropolis acceptances) needs
# the caller's RNG and stays on the host, on a few thousand gathered candidates; the O(N m D) distance passes and the Lloyd
# iterations run on the GPU (csrc/agp_kmeans.h).  Returns the same `Vector{Vector{T}}` the reference's constructors take.
function inducingpoints(alg::AGP.KmeansAlg, X::AbstractMatrix{T}; obsdim::Int=1, rng=Random.default_rng(),
                        nMarkov::Int=10, tol::Real=1e-3, maxiter::Int=100) where {T<:Union{Float32,Float64}}
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(X) : X)        # D x N == point-major
    D, N = size(Xd); m = alg.m
    m <= N || error("Input data not big enough given the desired number of inducing points")
    ctx = Ref{Ptr{Cvoid}}()
    st = ccall((:agp_ctx_create, libagp), Int32, (Int32, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), AMDGPU.device_id() - 1, AMDGPU.stream().stream, ctx)
    st == 0 || throw(AGPError(st, "agp_ctx_create"))
    dt = T == Float64 ? Int32(0) : Int32(1)
    try
        first = rand(rng, 1:N)
        c1 = Xd[:, first:first]
        d1 = ROCVector{T}(undef, N)
        check(ctx[], ccall((:agp_nearest_center, libagp), Int32,
                           (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Int32}, Ptr{Cvoid}),
                           ctx[], dt, pointer(Xd), N, D, D, pointer(c1), D, 1, C_NULL, pointer(d1)))
        q = Float64.(Array(d1)); q = q ./ sum(q) ./ 2 .+ 1 / (2N); q ./= sum(q)
        seeds = Matrix{Float64}(undef, D, m); seeds[:, 1] = Array(c1)
        Xh = nothing
        for i in 2:m                                           # one short Metropolis chain per further centre
            prop = sample(rng, 1:N, Weights(q), nMarkov)
            cand = Float64.(Array(Xd[:, prop]))
            dmin(v) = minimum(sum(abs2, seeds[:, 1:(i - 1)] .- v; dims=1))
            x = cand[:, 1]; dx = dmin(x)
            for j in 2:nMarkov
                yv = cand[:, j]; dy = dmin(yv)
                if dy > rand(rng) * dx
                    x, dx = yv, dy
                end
            end
            seeds[:, i] = x
        end
        Cd = ROCArray{T}(seeds)
        it, conv, obj = Ref{Int32}(), Ref{Int32}(), Ref{Float64}()
        check(ctx[], ccall((:agp_kmeans, libagp), Int32,
                           (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int32, Float64, Ptr{Int32},
                            Ptr{Int32}, Ref{Int32}, Ref{Float64}, Ref{Int32}),
                           ctx[], dt, pointer(Xd), N, D, D, pointer(Cd), D, m, maxiter, tol, C_NULL, C_NULL, it, obj, conv))
        Z = Array(Cd)
        return [Z[:, j] for j in 1:m]
    finally
        ccall((:agp_ctx_destroy, libagp), Int32, (Ptr{Cvoid},), ctx[])
    end
end

# ---- OnlineSVGP: streaming batches (src/models/OnlineSVGP.jl, src/training/onlinetraining.jl:17-218) ---------------------------
# A streaming model is a CHAIN of device handles: every arriving batch may grow Z (the reference's own InducingPoints.updateZ /
# remove_point run on the host, exactly where onlinetraining.jl:153-172 calls them), so a fresh handle is created for the new
# inducing points and the previous posterior is installed as its prior:
#   save_old_gp! (:170-180)          -> agp_svgp_online_snapshot  (invDₐ = Σₐ⁻¹ − Kₐ⁻¹, η₁ₐ, 𝓛ₐ read off the old handle)
#   compute_kernel_matrices (:199-237) -> agp_svgp_set_online_prior (K_ab, κₐ, K̃ₐ formed at the next K refresh)
#   first iteration (:78-104)        -> agp_svgp_online_first_step (local update under the OLD inducing points / posterior)
#   later iterations                 -> agp_svgp_cavi_step (full batch, closed-form natural parameters, analyticVI.jl:183-203)
# Only AnalyticVI() is accepted (the reference's stochastic branch uses an undefined name, onlinetraining.jl:52).  All latents of a
# handle share m: latents whose OIPS runs end with fewer points are filled with neutral far-away points (every kernel value that
# involves one is exactly 0), as the Python mirror does (augmentedgaussianprocesses.jl_amd/online.py, _pad_inducing).
mutable struct HipOnlineModel{T}
    model::AGP.OnlineSVGP{T}
    cur::Union{Nothing,HipModel}     # device twin of the current inducing points (an SVGP view of model.f)
    m_real::Vector{Int}
end
HipOnlineModel(m::AGP.OnlineSVGP{T}) where {T} = HipOnlineModel{T}(m, nothing, Int[])

const FAR = 1.0e6
function pad_inducing(Zs::Vector{<:AbstractVector})
    mmax = maximum(length, Zs)
    D = length(first(first(Zs)))
    return [vcat(collect.(Z), [fill(FAR * j, D) for j in 1:(mmax - length(Z))]) for Z in Zs], length.(Zs)
end

function train!(ho::HipOnlineModel{T}, X::AbstractMatrix, y::AbstractArray, state=nothing; iterations::Int=20,
                callback=nothing, obsdim::Int=1) where {T}
    iterations > 0 || error("Number of iterations should be positive")
    m = ho.model
    AGP.is_stochastic(m) && error("OnlineSVGP streams full batches on this path (onlinetraining.jl:48-53 cannot run)")
    Xv = KernelFunctions.vec_of_vecs(X; obsdim)
    first_batch = AGP.n_iter(m) == 0
    old = ho.cur
    snaps = nothing
    if first_batch
        AGP.init_online_model(m, Xv)                                          # onlinetraining.jl:182-197 (OIPS on the host)
    else
        pull_hypers!(old)                                                     # kernels / Z as the last hyper steps left them
        snaps = map(1:nlat(old)) do i                                         # save_old_gp!, :170-180
            mo = old.maxbatch; mm = AGP.dim(old.model.f[i])
            iD = ROCMatrix{T}(undef, mm, mm); e1 = ROCVector{T}(undef, mm); pl = Ref{Float64}()
            check(old.ctx, ccall((:agp_svgp_online_snapshot, libagp), Int32,
                                 (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ref{Float64}), old.h, i - 1, pointer(iD), mm, pointer(e1), pl))
            (iD, e1, pl[], reduce(hcat, AGP.Zview(old.model.f[i])))
        end
        for gp in m.f                                                         # remove_point (:172) then updateZ (:153-160)
            gp.Zₐ = deepcopy(gp.Z)
            gp.Z = AGP.InducingPoints.remove_point(Random.GLOBAL_RNG, gp.Z, gp.Zalg,
                                                   kernelmatrix(AGP.kernel(gp), gp.Z) + T(AGP.jitt) * I)
            gp.Z = AGP.InducingPoints.updateZ(gp.Z, gp.Zalg, Xv; kernel=AGP.kernel(gp))
            gp.post.dim = length(AGP.Zview(gp))
        end
    end
    Zs, m_real = pad_inducing([AGP.Zview(gp) for gp in m.f])
    # an SVGP view of the online latents (same kernels / optimisers, padded Z): what the device handle is created from
    view = SVGP(AGP.kernel.(m.f) |> first, AGP.likelihood(m), AnalyticVI(), Zs[1]; optimiser=AGP.opt(first(m.f)),
                Zoptimiser=AGP.Zopt(first(m.f)), atfrequency=m.atfrequency)
    for (gp, k, Z) in zip(view.f, AGP.kernel.(m.f), Zs)
        gp.prior.kernel = k; gp.Z = Z
    end
    new = HipModel(view)
    data = upload!(new, X, y; obsdim)
    B = new.N
    ensure_handle!(new, max(B, old === nothing ? 0 : old.maxbatch))
    mp = length(Zs[1])
    for i in 1:length(m.f)
        if first_batch                                                        # init_opt_state(::OnlineVarLatent), states.jl:85-97
            E = Matrix{T}(I, mp, mp); E[(m_real[i] + 1):end, (m_real[i] + 1):end] .= 0
            Ed = ROCArray(E); z = ROCArray(zeros(T, mp))
            check(new.ctx, ccall((:agp_svgp_set_online_prior, libagp), Int32,
                                 (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Float64),
                                 new.h, i - 1, C_NULL, 0, mp, pointer(Ed), mp, pointer(z), 0.0))
        else
            iD, e1, pl, Za = snaps[i]
            Zad = ROCArray{T}(Za)
            check(new.ctx, ccall((:agp_svgp_set_online_prior, libagp), Int32,
                                 (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Float64),
                                 new.h, i - 1, pointer(Zad), size(Za, 1), size(Za, 2), pointer(iD), size(iD, 1), pointer(e1), pl))
        end
    end
    start = 1
    if !first_batch      # first iteration: local update under the old inducing points, natural gradient under the new (:78-104)
        check(new.ctx, ccall((:agp_svgp_online_first_step, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
                             new.h, old.h, pointer(new.X), size(new.X, 1), pointer(new.y), B))
        start = 2
    end
    hyper_on = any(gp -> AGP.opt(gp) !== nothing || AGP.Zopt(gp) !== nothing, m.f)
    for it in 1:iterations
        it >= start && update_parameters!(new, nothing, 1.0)
        callback === nothing || callback(ho, new, AGP.n_iter(m))
        if hyper_on && AGP.n_iter(m) % m.atfrequency == 0 && AGP.n_iter(m) >= 3                     # :112-114
            update_hyperparameters!(new)
        end
        AGP.inference(m).n_iter += 1
    end
    check(new.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), new.h))
    check(new.ctx, ccall((:agp_svgp_refresh_K, libagp), Int32, (Ptr{Cvoid},), new.h))
    pull_posterior!(new); pull_hypers!(new)
    for (gp, vgp, n) in zip(m.f, view.f, m_real)                              # back into the reference object, padding stripped
        gp.post.μ = vgp.post.μ[1:n]; gp.post.Σ = Symmetric(Matrix(vgp.post.Σ)[1:n, 1:n])
        gp.post.η₁ = vgp.post.η₁[1:n]; gp.post.η₂ = Symmetric(Matrix(vgp.post.η₂)[1:n, 1:n])
        gp.Z = vgp.Z[1:n]
    end
    old === nothing || destroy!(old)
    ho.cur, ho.m_real = new, m_real
    AGP.set_trained!(m, true)
    return ho, new
end
predict_f(ho::HipOnlineModel, Xt::AbstractMatrix, state=nothing; kw...) = predict_f(ho.cur, Xt; kw...)
predict_f_grad(ho::HipOnlineModel, Xt::AbstractMatrix; kw...) = predict_f_grad(ho.cur, Xt; kw...)
predict_y(ho::HipOnlineModel, Xt::AbstractMatrix, state=nothing; kw...) = predict_y(ho.cur, Xt; kw...)
proba_y(ho::HipOnlineModel, Xt::AbstractMatrix, state=nothing; kw...) = proba_y(ho.cur, Xt; kw...)
objective(ho::HipOnlineModel, state=nothing, y=nothing) = objective(ho.cur)   # incl. −extraKL (KLdivergences.jl:30-54)

# ---- drop-in methods on the reference's own types ----------------------------------------------------------------------------------
# With the shim loaded, `train!(model, X, y, n)` on an SVGP / MOSVGP / OnlineSVGP with AnalyticVI / AnalyticSVI runs on the device:
# these methods are MORE SPECIFIC than the reference's `train!(model::AbstractGPModel, X::AbstractArray, y::AbstractArray, ...)`
# (src/training/training.jl:13-22) and `update_parameters!` entry (:140-144), so dispatch selects them -- no wrapper call at the
# user's site; `backend=:cpu` (or `AGPHip.default_backend!(:cpu)`) falls through to the reference's own method with `invoke`.
# The device twin of a model lives in a WeakKeyDict keyed by the model object; predictions, ELBO and objective look it up and fall
# back to the reference when the model was never trained on the device.  (As a package extension this section is
# `ext/AGPHipExt.jl`, triggered by `using AMDGPU`.)
const HipSVGP{T} = Union{SVGP{T,<:Any,<:AnalyticVI},AGP.MOSVGP{T,<:Any,<:AnalyticVI}}
const BACKEND = Ref(:hip)
default_backend!(b::Symbol) = (b in (:hip, :cpu) || throw(ArgumentError("backend is :hip or :cpu")); BACKEND[] = b)
const TWINS = WeakKeyDict{Any,Any}()
twin(model::HipSVGP; kw...) = get!(() -> HipModel(model; kw...), TWINS, model)
twin(model::AGP.OnlineSVGP) = get!(() -> HipOnlineModel(model), TWINS, model)
has_twin(model) = haskey(TWINS, model)

function train!(model::HipSVGP, X::AbstractArray, y::AbstractArray, iterations::Int=100; backend::Symbol=BACKEND[],
                reference_compat_stale_K::Bool=false, kwargs...)
    backend === :cpu &&
        return invoke(train!, Tuple{AGP.AbstractGPModel,AbstractArray,AbstractArray,Int}, model, X, y, iterations; kwargs...)
    hm = twin(model; reference_compat_stale_K)
    _, state = train!(hm, X, y, iterations; kwargs...)      # leaves the trained posterior / kernels / Z in `model` as well
    return model, state
end
function train!(model::AGP.OnlineSVGP{T,<:Any,<:AnalyticVI}, X::AbstractMatrix, y::AbstractArray, state=nothing;
                backend::Symbol=BACKEND[], kwargs...) where {T}
    backend === :cpu &&
        return invoke(train!, Tuple{AGP.OnlineSVGP,AbstractMatrix,AbstractArray,Any}, model, X, y, state; kwargs...)
    _, st = train!(twin(model), X, y, state; kwargs...)
    return model, st
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::Union{HipSVGP,AGP.OnlineSVGP}, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
function ELBO(model::HipSVGP, X::AbstractMatrix, y::AbstractArray; backend::Symbol=BACKEND[], kw...)
    (backend === :cpu || !has_twin(model)) && return invoke(ELBO, Tuple{AGP.AbstractGPModel,AbstractMatrix,AbstractArray}, model, X, y; kw...)
    return ELBO(TWINS[model], X, y; kw...)
end
objective(model::HipSVGP, state::HipModel, y=nothing) = objective(state)    # the state train! returned IS the device twin

# VGP{T,L,<:AnalyticVI} (src/models/VGP.jl): train!(model, iterations) on the model's own data (training.jl:113-120) through the
# same ABI, on a handle created with AGP_FLAG_FULL; predictions and the ELBO look the twin up like the sparse models'.
const HipVGP{T} = AGP.VGP{T,<:Any,<:AnalyticVI}
twin(model::HipVGP) = get!(() -> HipModel(model), TWINS, model)
function train!(model::HipVGP, iterations::Int; backend::Symbol=BACKEND[], kwargs...)
    backend === :cpu && return invoke(train!, Tuple{AGP.AbstractGPModel,Int}, model, iterations; kwargs...)
    X = reduce(hcat, AGP.input(model.data))'                     # N x D
    _, state = train!(twin(model), X, AGP.output(model.data), iterations; kwargs...)
    return model, state
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::HipVGP, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
objective(model::HipVGP, state::HipModel, y=nothing) = objective(state)

# VGP{T,L,<:QuadratureVI} (src/inference/numericalVI.jl, quadratureVI.jl): the same train!(model, iterations) on a handle created with
# AGP_FLAG_FULL | AGP_FLAG_NUMERICAL, which keeps (mu, Sigma) and the optimiser's moments; every iteration is one
# agp_svgp_nvi_step (update_parameters! above), objective(model, state, y) the quadrature ELBO (agp_svgp_elbo).  Three definitions of
# the reference are restated in their intended form on the device (agp_hip.h, "NUMERICAL INFERENCE"): the CPU backend keeps its own.
const HipQVGP{T} = AGP.VGP{T,<:Any,<:AGP.QuadratureVI}
twin(model::HipQVGP) = get!(() -> HipModel(model), TWINS, model)
# SVGP{T,L,<:QuadratureVI} (QuadratureVI and QuadratureSVI): train!(model, X, y, iterations) is the sparse models' own method
# (HipSVGP above takes every SVGP); its steps go to agp_svgp_nvi_step with the minibatch indices and rho = N / B
# (update_parameters!), the handle is created with AGP_FLAG_NUMERICAL alone, the posterior comes back as (mu, Sigma).
const HipQSVGP{T} = SVGP{T,<:Any,<:AGP.QuadratureVI}
nvi_info(model::HipQSVGP) = nvi_info_of(TWINS[model])
twin(model::HipQSVGP) = get!(() -> HipModel(model), TWINS, model)
function train!(model::HipQSVGP, X::AbstractArray, y::AbstractArray, iterations::Int=100; backend::Symbol=BACKEND[], kwargs...)
    backend === :cpu &&
        return invoke(train!, Tuple{AGP.AbstractGPModel,AbstractArray,AbstractArray,Int}, model, X, y, iterations; kwargs...)
    _, state = train!(twin(model), X, y, iterations; kwargs...)
    return model, state
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::HipQSVGP, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
objective(model::HipQSVGP, state::HipModel, y=nothing) = objective(state)
# x_j = sqrt(2) t_j, w_j = omega_j / sqrt(pi) (quadratureVI.jl:36-40: the inference object holds them ready-made) and the optimiser
function nvi_configure!(hm::HipModel)
    inf = AGP.inference(hm.model)
    o = inf.vi_opt[1].optimiser
    kind, p1, p2, ϵ = o isa Optimisers.ADAM ? (0, Float64(o.beta[1]), Float64(o.beta[2]), 1e-8) :
                      o isa Optimisers.Descent ? (1, 0.0, 0.0, 0.0) :
                      o isa Optimisers.Momentum ? (2, Float64(o.rho), 0.0, 0.0) :
                      error("QuadratureVI optimiser $(typeof(o)) is not available on the device (ADAM, Descent, Momentum are)")
    x, w = Vector{Float64}(inf.nodes), Vector{Float64}(inf.weights)
    check(hm.ctx, ccall((:agp_svgp_nvi_configure, libagp), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Float64, Float64, Float64),
                        hm.h, length(x), x, w, AGP.isnatural(inf) ? 1 : 0, kind, Float64(o.eta), p1, p2, ϵ))
    return hm
end
# ---- Monte-Carlo integration (MCIntegrationVI / MCIntegrationSVI, src/inference/MCVI.jl): the entry points of a handle created with
# AGP_FLAG_NUMERICAL | AGP_FLAG_MC (likelihood AGP_LIK_SOFTMAX or the LogisticSoftMax one, n_latent = K) and the two context-level ones.
# The table of normals of step t is a function of (seed, t) alone (agp_hip.h, "MC INTEGRATION"); nvi_step, nvi_info(latent) and
# nvi_state(latent) then work per latent.  The models of the reference are not yet dispatched onto these handles by this shim.
function mcvi_configure!(hm::HipModel, seed::Integer)
    inf = AGP.inference(hm.model)
    o = inf.vi_opt[1].optimiser
    kind, p1, p2, ϵ = o isa Optimisers.ADAM ? (0, Float64(o.beta[1]), Float64(o.beta[2]), 1e-8) :
                      o isa Optimisers.Descent ? (1, 0.0, 0.0, 0.0) :
                      o isa Optimisers.Momentum ? (2, Float64(o.rho), 0.0, 0.0) :
                      error("MCIntegrationVI optimiser $(typeof(o)) is not available on the device (ADAM, Descent, Momentum are)")
    check(hm.ctx, ccall((:agp_svgp_mcvi_configure, libagp), Int32,
                        (Ptr{Cvoid}, Int32, UInt64, Int32, Int32, Float64, Float64, Float64, Float64),
                        hm.h, inf.nMC, UInt64(seed), AGP.isnatural(inf) ? 1 : 0, kind, Float64(o.eta), p1, p2, ϵ))
    return hm
end
# eps[nMC, K] of (seed, t, stream): stream 2 the gradient draw of step t, stream 3 the ELBO after t steps
function mc_normals(hm::HipModel, seed::Integer, t::Integer, stream::Integer, nMC::Integer, K::Integer)
    ctx = ensure_ctx!(hm)
    out = ROCMatrix{Float64}(undef, K, nMC)                      # (column-major K x nMC = the library's double[nMC][K])
    check(ctx, ccall((:agp_mc_normals, libagp), Int32, (Ptr{Cvoid}, UInt64, Int64, Int32, Int32, Int32, Ptr{Cvoid}),
                     ctx, UInt64(seed), t, stream, nMC, K, pointer(out)))
    return permutedims(Array(out))
end
# (ell [n], g [n x K], h [n x K]) of the expectation kernel on given moments mu, var [n x K]; y_class 0-based
function mc_expectations(hm::HipModel, lik::LikDesc, y_class::AbstractVector{<:Integer}, mu::AbstractMatrix, var::AbstractMatrix,
                         nMC::Integer, seed::Integer, t::Integer, stream::Integer=2)
    ctx = ensure_ctx!(hm)
    n, K = size(mu)
    yd, md, vd = ROCVector{Int32}(y_class), ROCMatrix{Float64}(mu), ROCMatrix{Float64}(var)   # (column-major n x K = double[K][n])
    ell, g, h = ROCVector{Float64}(undef, n), similar(md), similar(md)
    check(ctx, ccall((:agp_mc_expectations, libagp), Int32,
                     (Ptr{Cvoid}, Ref{LikDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Int32, UInt64, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx, lik, pointer(yd), pointer(md), pointer(vd), n, K, nMC, UInt64(seed), t, stream, pointer(ell), pointer(g), pointer(h)))
    return Array(ell), Array(g), Array(h)
end
# (mu, Sigma) of the device -> the reference object; the natural parameters follow from them (posterior.jl)
function pull_nvi_posterior!(hm::HipModel{T}) where {T}
    gp = latents(hm.model)[1]
    m = AGP.dim(gp)
    μ = ROCVector{T}(undef, m); Σ = ROCMatrix{T}(undef, m, m)
    check(hm.ctx, ccall((:agp_svgp_get_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, 0, pointer(μ), pointer(Σ), C_NULL, C_NULL))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    gp.post.μ .= Array(μ)
    gp.post.Σ.data .= Array(Σ)
    return hm
end
# (alpha of the last step, halvings, rejected updates) of the backtracking since the handle was created
nvi_info(model::HipQVGP) = nvi_info_of(TWINS[model])
function nvi_info_of(hm::HipModel)
    a = Ref{Float64}(); hv = Ref{Int64}(); rj = Ref{Int64}()
    check(hm.ctx, ccall((:agp_svgp_nvi_info, libagp), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}, Ref{Int64}, Ref{Int64}), hm.h, 0, a, hv, rj))
    return a[], hv[], rj[]
end
function train!(model::HipQVGP, iterations::Int; backend::Symbol=BACKEND[], kwargs...)
    backend === :cpu && return invoke(train!, Tuple{AGP.AbstractGPModel,Int}, model, iterations; kwargs...)
    X = reduce(hcat, AGP.input(model.data))'                     # N x D
    _, state = train!(twin(model), X, AGP.output(model.data), iterations; kwargs...)
    return model, state
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::HipQVGP, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
objective(model::HipQVGP, state::HipModel, y=nothing) = objective(state)

# MOVGP{T,L,<:AnalyticVI} (src/models/MOVGP.jl): the multi-output full model, train!(model, iterations) on its own data; the handle
# is created with AGP_FLAG_FULL and the multi-output likelihood (is_full and is_mo both hold: the inputs of every latent are the
# training inputs, the targets go up point-major, A travels through agp_svgp_set_multioutput / agp_svgp_get_A as for MOSVGP).
const HipMOVGP{T} = AGP.MOVGP{T,<:Any,<:AnalyticVI}
twin(model::HipMOVGP) = get!(() -> HipModel(model), TWINS, model)
function train!(model::HipMOVGP, iterations::Int; backend::Symbol=BACKEND[], kwargs...)
    backend === :cpu && return invoke(train!, Tuple{AGP.AbstractGPModel,Int}, model, iterations; kwargs...)
    X = reduce(hcat, AGP.input(model.data))'                     # N x D
    _, state = train!(twin(model), X, AGP.output(model.data), iterations; kwargs...)
    return model, state
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::HipMOVGP, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
objective(model::HipMOVGP, state::HipModel, y=nothing) = objective(state)

# GP{T,<:GaussianLikelihood,<:Analytic} (src/models/GP.jl): exact regression on a handle created with AGP_FLAG_FULL | AGP_FLAG_EXACT.
# The posterior comes back as (alpha, Sigma) -- agp_svgp_get_state with eta1 = eta2 = NULL -- and log p is the handle's ELBO.
const HipGP{T} = AGP.GP{T,<:GaussianLikelihood,<:AGP.Analytic}
twin(model::HipGP) = get!(() -> HipModel(model), TWINS, model)
function pull_gp_posterior!(hm::HipModel{T}) where {T}
    f = only(latents(hm.model))
    N = AGP.dim(f)
    α, Σ = ROCArray{T}(undef, N), ROCArray{T}(undef, N, N)
    check(hm.ctx, ccall((:agp_svgp_get_state, libagp), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, 0, pointer(α), pointer(Σ), C_NULL, C_NULL))
    AMDGPU.synchronize()
    f.post.α = Array(α)
    f.post.Σ = cholesky(Symmetric(Array(Σ)))   # Posterior.Σ is a Cholesky{T,Matrix{T}} (posterior.jl:8-12)
    return nothing
end
function train!(model::HipGP, iterations::Int; backend::Symbol=BACKEND[], kwargs...)
    backend === :cpu && return invoke(train!, Tuple{AGP.AbstractGPModel,Int}, model, iterations; kwargs...)
    X = reduce(hcat, AGP.input(model.data))'                     # N x D
    _, state = train!(twin(model), X, AGP.output(model.data), iterations; kwargs...)
    return model, state
end
for f in (:predict_f, :predict_y, :proba_y)
    @eval function $f(model::HipGP, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...)
        (backend === :cpu || !has_twin(model)) &&
            return invoke($f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; kw...)
        return $f(TWINS[model], X_test; kw...)
    end
end
objective(model::HipGP, state::HipModel, y=nothing) = objective(state)
objective(model::HipGP, state, y) = has_twin(model) ? objective(TWINS[model]) : AGP.log_py(model, y)
ELBO(model::HipGP) = has_twin(model) ? objective(TWINS[model]) : AGP.log_py(model, AGP.output(model.data))

# MCGP{T,L,<:GibbsSampling} (src/models/MCGP.jl, src/training/sampling.jl): sample(model, n) on a handle created with
# AGP_FLAG_FULL | AGP_FLAG_SAMPLED.  The whole chain is enqueued by agp_svgp_gibbs_sample; the kept samples come back as the
# reference's sample_store (a vector over samples of a vector over latents of f), which the predictors read through
# agp_svgp_predict_samples.  `seed` (default: drawn from Random.GLOBAL_RNG at the first call) and the sweep counter of the handle make
# successive calls one chain (cat = true).  Never run: there is no Julia toolchain in the test environment.
const HipMCGP{T} = AGP.MCGP{T,<:Any,<:AGP.GibbsSampling}
const MCGP_SEED = IdDict{Any,UInt64}()
twin(model::HipMCGP) = get!(() -> HipModel(model), TWINS, model)
function sample(model::HipMCGP{T}, N::Int; thinning::Int=AGP.inference(model).thinning, discard_initial::Int=AGP.inference(model).nBurnin,
                cat::Bool=true, seed=nothing, backend::Symbol=BACKEND[], kwargs...) where {T}
    backend === :cpu && return invoke(sample, Tuple{AGP.MCGP,Int}, model, N; thinning, discard_initial, cat, kwargs...)
    hm = twin(model)
    X = reduce(hcat, AGP.input(model.data))'                     # N x D
    hm.X === nothing && upload!(hm, X, AGP.output(model.data))
    ensure_handle!(hm, hm.N)
    s = seed === nothing ? get!(() -> rand(UInt64), MCGP_SEED, model) : (MCGP_SEED[model] = UInt64(seed))
    store = ROCMatrix{T}(undef, hm.N, N)                         # column k == kept sample k (ABI: T[n_samples][lds])
    check(hm.ctx, ccall((:agp_svgp_gibbs_sample, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, UInt64, Ptr{Cvoid}, Int64),
                        hm.h, pointer(hm.y), N, discard_initial, thinning, s, pointer(store), hm.N))
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    F = Array(store)
    samples = [[F[:, k]] for k in 1:N]
    inf = AGP.inference(model)
    inf.n_iter += discard_initial + 1 + (N - 1) * thinning
    inf.sample_store = (!cat || isempty(inf.sample_store)) ? samples : vcat(inf.sample_store, samples)   # bundle_samples, sampling.jl:77-88
    only(model.f).post.f .= F[:, end]
    return samples
end
function sweep_counter(model::HipMCGP)
    t = Ref{Int64}(0)
    hm = twin(model)
    check(hm.ctx, ccall((:agp_svgp_gibbs_counter, libagp), Int32, (Ptr{Cvoid}, Int32, Ref{Int64}), hm.h, 0, t))
    return t[]
end
# sample_local! on given f outside any model: theta (and omega of the StudentT likelihood) for (seed, t)
function sample_local(hm::HipModel{T}, lik, y::AbstractVector, f::AbstractVector, seed::Integer, t::Integer=0) where {T}
    ctx = ensure_ctx!(hm)
    yd, fd = ROCVector{Float64}(y), ROCVector{Float64}(f)
    θ, aux = similar(fd), similar(fd)
    check(ctx, ccall((:agp_sample_local, libagp), Int32,
                     (Ptr{Cvoid}, Ref{LikDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, UInt64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx, lik_desc(lik), pointer(yd), pointer(fd), length(fd), UInt64(seed), t, pointer(θ), pointer(aux)))
    return Array(θ), Array(aux)
end
# mode 0: mean f*; 1: mean and variance (predictions.jl:94-118, intended form); 2: mean and variance of logistic(f*) (:266-276)
function _predict_samples(model::HipMCGP{T}, X_test::AbstractMatrix, mode::Int; obsdim::Int=1) where {T}
    hm = twin(model)
    store = AGP.inference(model).sample_store
    isempty(store) && error("the model holds no samples yet: call sample(model, n) first")
    ensure_handle!(hm, hm.N)
    Sd = ROCMatrix{T}(reduce(hcat, first.(store)))               # N x n_samples
    Xd = ROCArray{T}(obsdim == 1 ? permutedims(X_test) : X_test)
    D, nt = size(Xd)
    o0, o1 = ROCVector{T}(undef, nt), ROCVector{T}(undef, nt)
    check(hm.ctx, ccall((:agp_svgp_predict_samples, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                        hm.h, pointer(Xd), D, nt, pointer(Sd), size(Sd, 1), size(Sd, 2), mode, pointer(o0), mode == 0 ? C_NULL : pointer(o1)))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    return Array(o0), Array(o1)
end
function predict_f(model::HipMCGP, X_test::AbstractMatrix, state=nothing; cov::Bool=false, diag::Bool=true, backend::Symbol=BACKEND[], kw...)
    (backend === :cpu || !has_twin(model)) &&
        return invoke(predict_f, Tuple{AGP.AbstractGPModel,AbstractMatrix,Any}, model, X_test, state; cov, diag, kw...)
    cov && !diag && error("MCGP: the full covariance over the samples is not formed on the device")
    μ, σ² = _predict_samples(model, X_test, cov ? 1 : 0; kw...)
    return cov ? (μ, σ²) : μ
end
function proba_y(model::HipMCGP{T,<:AGP.BernoulliLikelihood}, X_test::AbstractMatrix, state=nothing; backend::Symbol=BACKEND[], kw...) where {T}
    (backend === :cpu || !has_twin(model)) &&
        return invoke(proba_y, Tuple{AGP.MCGP,AbstractMatrix,Any}, model, X_test, state; kw...)
    return _predict_samples(model, X_test, 2; kw...)
end
objective(model::HipMCGP, state::HipModel, y=nothing) = NaN      # MCGP.jl:91

# ---- pathwise posterior sampling (include/agp_hip.h, "PATHWISE SAMPLING") ---------------------------------------------------------
# paths = sample_paths(model, n; n_features=1024, seed=nothing, t=0) draws n functions from the posterior of a trained SVGP, VGP or GP
# (its device twin must exist: train with the :hip backend first); paths(X_test) evaluates them at any number of points: n x n_t, or
# a vector of such matrices, one per latent.  The draw is a snapshot on the device: training the model further does not change it.
# Everything random is a function of (seed, t, latent), as the header states.  Never run: there is no Julia toolchain in the test
# environment.
mutable struct PathwiseSamples
    p::Ptr{Cvoid}
    ctx::Ptr{Cvoid}
    hm::Any                                                      # keeps the context alive
    n_latent::Int
    n_features::Int
    n_samples::Int
    m::Int
    D::Int
    seed::UInt64
    t::Int64
end
const PATHWISE_SEED = IdDict{Any,UInt64}()
function free!(ps::PathwiseSamples)
    ps.p == C_NULL || ccall((:agp_pathwise_destroy, libagp), Int32, (Ptr{Cvoid},), ps.p)
    ps.p = C_NULL
    return nothing
end
function sample_paths(hm::HipModel, n::Integer; n_features::Integer=1024, seed=nothing, t::Integer=0)
    hm.h == C_NULL && error("sample_paths: the model has no device handle yet (train it with the :hip backend first)")
    s = seed === nothing ? get!(() -> rand(UInt64), PATHWISE_SEED, hm) : UInt64(seed)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(hm.ctx, ccall((:agp_svgp_pathwise_draw, libagp), Int32, (Ptr{Cvoid}, Int32, Int32, UInt64, Int64, Ref{Ptr{Cvoid}}),
                        hm.h, n_features, n, s, t, p))
    nl, nf, ns, m, D = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(hm.ctx, ccall((:agp_pathwise_info, libagp), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int64}, Ref{Int64}),
                        p[], nl, nf, ns, m, D))
    ps = PathwiseSamples(p[], hm.ctx, hm, nl[], nf[], ns[], m[], D[], s, t)
    finalizer(free!, ps)
    return ps
end
sample_paths(model::AGP.AbstractGPModel, n::Integer; kw...) =
    has_twin(model) ? sample_paths(TWINS[model], n; kw...) : error("sample_paths: train the model with the :hip backend first")
function (ps::PathwiseSamples)(X_test::AbstractMatrix; obsdim::Int=1)
    ps.p == C_NULL && error("the paths have been freed")
    Xd = ROCArray{Float64}(obsdim == 1 ? permutedims(X_test) : X_test)   # D x n_t column-major == point-major
    D, nt = size(Xd)
    out = ROCArray{Float64}(undef, nt, ps.n_samples, ps.n_latent)        # column-major == double[n_latent][n_samples][n_t]
    check(ps.ctx, ccall((:agp_pathwise_eval, libagp), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64),
                        ps.p, pointer(Xd), D, nt, pointer(out), max(nt, 1)))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), ps.ctx)
    F = Array(out)
    paths = [permutedims(F[:, :, l]) for l in 1:ps.n_latent]             # n_samples x n_t per latent
    return ps.n_latent == 1 ? only(paths) : paths
end
# pathwise_grad(paths, X_test; value=false): d f_s / d x at the test points, n_samples x n_t x D per latent (a vector over latents for
# several); value=true returns (F, G) with F what paths(X_test) returns.  agp_pathwise_eval_grad; refused for the ExponentialKernel.
function pathwise_grad(ps::PathwiseSamples, X_test::AbstractMatrix; value::Bool=false, obsdim::Int=1)
    ps.p == C_NULL && error("the paths have been freed")
    Xd = ROCArray{Float64}(obsdim == 1 ? permutedims(X_test) : X_test)   # D x n_t column-major == point-major
    D, nt = size(Xd)
    g = ROCArray{Float64}(undef, D, nt, ps.n_samples, ps.n_latent)       # column-major == double[n_latent][n_samples][n_t][D]
    f = value ? ROCArray{Float64}(undef, nt, ps.n_samples, ps.n_latent) : nothing
    check(ps.ctx, ccall((:agp_pathwise_eval_grad, libagp), Int32,
                        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64),
                        ps.p, pointer(Xd), D, nt, value ? pointer(f) : C_NULL, max(nt, 1), pointer(g), max(nt, 1), D))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), ps.ctx)
    Gh = Array(g)
    grads = [permutedims(Gh[:, :, :, l], (3, 2, 1)) for l in 1:ps.n_latent]   # n_samples x n_t x D per latent
    G = ps.n_latent == 1 ? only(grads) : grads
    value || return G
    Fh = Array(f)
    paths = [permutedims(Fh[:, :, l]) for l in 1:ps.n_latent]
    return (ps.n_latent == 1 ? only(paths) : paths), G
end
# pathwise_maximize(paths, X0, lo, hi; steps=100, lr=nothing, ...): multi-start ADAM ascent of every path on the device, one launch
# (agp_pathwise_maximize).  X0 is R x D (the same starts for every path) or n_samples x R x D; lo, hi and lr are scalars or vectors of
# length D, lr=nothing the interface default 0.02 (hi - lo).  Returns (x_best n_samples x D, f_best n_samples); full=true returns
# (x_best, f_best, idx (1-based), X n_samples x R x D, F n_samples x R).  The struct mirrors agp_pw_ascent_opts field by field.
# Never run: there is no Julia toolchain in the test environment.
struct PwAscentOpts
    steps::Int32
    minimize::Int32
    x0_shared::Int32
    beta1::Float64
    beta2::Float64
    eps::Float64
    lo_host::Ptr{Float64}
    hi_host::Ptr{Float64}
    lr_host::Ptr{Float64}
end
function pathwise_maximize(ps::PathwiseSamples, X0::AbstractArray, lo, hi; steps::Integer=100, lr=nothing, beta1::Real=0.9,
                           beta2::Real=0.999, eps::Real=1e-8, latent::Integer=1, minimize::Bool=false, full::Bool=false)
    ps.p == C_NULL && error("the paths have been freed")
    D, S = ps.D, ps.n_samples
    shared = ndims(X0) == 2
    (shared ? size(X0, 2) == D : (ndims(X0) == 3 && size(X0, 1) == S && size(X0, 3) == D)) ||
        error("pathwise_maximize: X0 must be R x $D or $S x R x $D")
    R = shared ? size(X0, 1) : size(X0, 2)
    vec_of(v) = v isa Number ? fill(Float64(v), D) : collect(Float64, v)
    lov, hiv = vec_of(lo), vec_of(hi)
    lrv = lr === nothing ? map(w -> w == 0 ? 1.0 : 0.02 * w, hiv .- lov) : vec_of(lr)
    (length(lov) == D && length(hiv) == D && length(lrv) == D) || error("pathwise_maximize: lo, hi and lr must be scalars or of length $D")
    Xd = ROCArray{Float64}(shared ? permutedims(X0) : permutedims(X0, (3, 2, 1)))   # column-major D x R (x S) == [s][r][d]
    X = ROCArray{Float64}(undef, D, R, S)
    F = ROCArray{Float64}(undef, R, S)
    xb = ROCArray{Float64}(undef, D, S)
    fb = ROCArray{Float64}(undef, S)
    ib = ROCArray{Int64}(undef, S)
    GC.@preserve lov hiv lrv begin
        opts = Ref(PwAscentOpts(steps, minimize ? 1 : 0, shared ? 1 : 0, beta1, beta2, eps, pointer(lov), pointer(hiv), pointer(lrv)))
        check(ps.ctx, ccall((:agp_pathwise_maximize, libagp), Int32,
                            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Int64, Ref{PwAscentOpts}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid},
                             Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                            ps.p, latent - 1, pointer(Xd), D, R, opts, full ? pointer(X) : C_NULL, D, full ? pointer(F) : C_NULL, R,
                            pointer(xb), D, pointer(fb), pointer(ib)))
    end
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), ps.ctx)
    x_best, f_best = permutedims(Array(xb)), Array(fb)
    full || return x_best, f_best
    return x_best, f_best, Array(ib) .+ 1, permutedims(Array(X), (3, 2, 1)), permutedims(Array(F))
end
# the tables of one latent (0-based `which`: 0 omega l x D, 1 phase l, 2 W l x S, 3 V m x S, 4 E m x S), as Julia matrices
function pathwise_table(ps::PathwiseSamples, which::Integer; latent::Integer=1)
    rows, cols = which == 0 ? (ps.n_features, ps.D) : which == 1 ? (ps.n_features, 1) :
                 which == 2 ? (ps.n_features, ps.n_samples) : (ps.m, ps.n_samples)
    buf = ROCMatrix{Float64}(undef, cols, rows)                          # column-major cols x rows == the library's rows x cols
    check(ps.ctx, ccall((:agp_pathwise_get, libagp), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Int64),
                        ps.p, latent - 1, which, pointer(buf), cols))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), ps.ctx)
    return permutedims(Array(buf))
end
# the spectral draw alone, outside any model: (omega l x D, phase l)
function pathwise_features(hm::HipModel, k::Kernel, D::Integer, n_features::Integer, seed::Integer, t::Integer=0; latent::Integer=1)
    ctx = ensure_ctx!(hm)
    om, ph = ROCMatrix{Float64}(undef, D, n_features), ROCVector{Float64}(undef, n_features)
    kd, keep = kernel_desc(k, Int(D))
    GC.@preserve keep check(ctx, ccall((:agp_pathwise_features, libagp), Int32,
                                       (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int32, UInt64, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                                       ctx, kd, D, n_features, UInt64(seed), t, latent - 1, pointer(om), pointer(ph)))
    return permutedims(Array(om)), Array(ph)
end

# ---- acquisition functions (include/agp_hip.h, "ACQUISITION FUNCTIONS"; no counterpart in the reference) ------------------------------
# UCB(beta), EI(best, xi), PI(best, xi), LogEI(best, xi), LogPI(best, xi) of the moments of predict_f, Float64 single-output models;
# minimize=true: the objective is minimised (the acquisition value itself is always maximised).  The struct mirrors agp_acq_desc field
# by field.
# Never run: there is no Julia toolchain in the test environment.
struct AcqDesc
    kind::Int32
    minimize::Int32
    beta::Float64
    best::Float64
    xi::Float64
end
UCB(beta::Real=2.0; minimize::Bool=false) = AcqDesc(0, minimize ? 1 : 0, beta, 0.0, 0.0)
EI(best::Real, xi::Real=0.0; minimize::Bool=false) = AcqDesc(1, minimize ? 1 : 0, 0.0, best, xi)
PI(best::Real, xi::Real=0.0; minimize::Bool=false) = AcqDesc(2, minimize ? 1 : 0, 0.0, best, xi)
# the same two in logarithms (AGP_ACQ_LOG = 4 set on the kind): finite with a useful gradient where EI and PI have underflowed to 0
LogEI(best::Real, xi::Real=0.0; minimize::Bool=false) = AcqDesc(5, minimize ? 1 : 0, 0.0, best, xi)
LogPI(best::Real, xi::Real=0.0; minimize::Bool=false) = AcqDesc(6, minimize ? 1 : 0, 0.0, best, xi)
# acquisition(hm, acq, X; grad=false, latent=1): alpha at the rows of X (n_t), with grad=true (alpha, G n_t x D)
function acquisition(hm::HipModel{Float64}, acq::AcqDesc, X::AbstractMatrix; grad::Bool=false, latent::Integer=1, obsdim::Int=1)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd = ROCArray{Float64}(obsdim == 1 ? permutedims(X) : X)
    D, nt = size(Xd)
    a = ROCArray{Float64}(undef, nt)
    G = grad ? ROCArray{Float64}(undef, D, nt) : nothing     # column-major D x n_t == the ABI's [n_t][ldg = D]
    check(hm.ctx, ccall((:agp_svgp_acquisition, libagp), Int32,
                        (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                        hm.h, latent - 1, Ref(acq), pointer(Xd), D, nt, pointer(a), grad ? pointer(G) : C_NULL, D))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    return grad ? (Array(a), permutedims(Array(G))) : Array(a)
end
# acquisition_moments(hm, acq, mu, var): the point function alone, (alpha, d alpha / d mu, d alpha / d var)
function acquisition_moments(hm::HipModel, acq::AcqDesc, mu::AbstractVector, var::AbstractVector)
    ctx = ensure_ctx!(hm)
    n = length(mu)
    md, vd = ROCArray{Float64}(mu), ROCArray{Float64}(var)
    a, dm, dv = (ROCArray{Float64}(undef, n) for _ in 1:3)
    check(ctx, ccall((:agp_acq_moments, libagp), Int32,
                     (Ptr{Cvoid}, Ref{AcqDesc}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx, Ref(acq), n, pointer(md), pointer(vd), pointer(a), pointer(dm), pointer(dv)))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), ctx)
    return Array(a), Array(dm), Array(dv)
end
# maximize_acquisition(hm, acq, X0, lo, hi; steps=100, lr=nothing, ...): multi-start ADAM ascent on the device (agp_svgp_acq_maximize).
# X0 is R x D; lo, hi and lr as in pathwise_maximize.  Returns (x_best (D), a_best); full=true (x_best, a_best, idx (1-based), X R x D,
# A (R)).
function maximize_acquisition(hm::HipModel{Float64}, acq::AcqDesc, X0::AbstractMatrix, lo, hi; steps::Integer=100, lr=nothing,
                              beta1::Real=0.9, beta2::Real=0.999, eps::Real=1e-8, latent::Integer=1, full::Bool=false)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    R, D = size(X0)
    vec_of(v) = v isa Number ? fill(Float64(v), D) : collect(Float64, v)
    lov, hiv = vec_of(lo), vec_of(hi)
    lrv = lr === nothing ? map(w -> w == 0 ? 1.0 : 0.02 * w, hiv .- lov) : vec_of(lr)
    (length(lov) == D && length(hiv) == D && length(lrv) == D) || error("maximize_acquisition: lo, hi and lr must be scalars or of length $D")
    Xd = ROCArray{Float64}(permutedims(X0))                  # column-major D x R == [r][d]
    X, A = ROCArray{Float64}(undef, D, R), ROCArray{Float64}(undef, R)
    xb, ab, ib = ROCArray{Float64}(undef, D), ROCArray{Float64}(undef, 1), ROCArray{Int64}(undef, 1)
    GC.@preserve lov hiv lrv begin
        opts = Ref(PwAscentOpts(steps, 0, 0, beta1, beta2, eps, pointer(lov), pointer(hiv), pointer(lrv)))
        check(hm.ctx, ccall((:agp_svgp_acq_maximize, libagp), Int32,
                            (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Ref{PwAscentOpts}, Ptr{Cvoid}, Int64, Ptr{Cvoid},
                             Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                            hm.h, latent - 1, Ref(acq), pointer(Xd), D, R, opts, full ? pointer(X) : C_NULL, D, full ? pointer(A) : C_NULL,
                            pointer(xb), pointer(ab), pointer(ib)))
    end
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    x_best, a_best = Array(xb), Array(ab)[1]
    full || return x_best, a_best
    return x_best, a_best, Array(ib)[1] + 1, permutedims(Array(X)), Array(A)
end
# Pending points ("ACQUISITION FUNCTIONS", paragraph "Pending points"): the posterior conditioned on P (n x D) at its own predicted mean
# with the noise variance pending_noise; the mean stays, the variance shrinks.  Never run, like everything in this file.
# acquisition_pending(hm, acq, X, P; pending_noise=0.0, grad=false, latent=1): alpha_P at the rows of X (agp_svgp_acquisition_pending)
function acquisition_pending(hm::HipModel{Float64}, acq::AcqDesc, X::AbstractMatrix, P::AbstractMatrix; pending_noise::Real=0.0,
                             grad::Bool=false, latent::Integer=1)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    Xd, Pd = ROCArray{Float64}(permutedims(X)), ROCArray{Float64}(permutedims(P))   # column-major D x n == [i][d]
    D, nt = size(Xd)
    n = size(Pd, 2)
    a = ROCArray{Float64}(undef, nt)
    G = grad ? ROCArray{Float64}(undef, D, nt) : nothing
    check(hm.ctx, ccall((:agp_svgp_acquisition_pending, libagp), Int32,
                        (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Float64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid},
                         Int64),
                        hm.h, latent - 1, Ref(acq), n > 0 ? pointer(Pd) : C_NULL, D, n, pending_noise, pointer(Xd), D, nt, pointer(a),
                        grad ? pointer(G) : C_NULL, D))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    return grad ? (Array(a), permutedims(Array(G))) : Array(a)
end
# maximize_acquisition_batch(hm, acq, q, X0, lo, hi; pending=nothing, pending_noise=0.0, steps=100, ...): q points picked greedily on
# the device (agp_svgp_acq_maximize_batch), each round conditioned on `pending` and on the winners before.  Returns (X_batch q x D,
# a_batch (q)); full=true adds idx (q, 1-based).
function maximize_acquisition_batch(hm::HipModel{Float64}, acq::AcqDesc, q::Integer, X0::AbstractMatrix, lo, hi; pending=nothing,
                                    pending_noise::Real=0.0, steps::Integer=100, lr=nothing, beta1::Real=0.9, beta2::Real=0.999,
                                    eps::Real=1e-8, latent::Integer=1, full::Bool=false)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    R, D = size(X0)
    vec_of(v) = v isa Number ? fill(Float64(v), D) : collect(Float64, v)
    lov, hiv = vec_of(lo), vec_of(hi)
    lrv = lr === nothing ? map(w -> w == 0 ? 1.0 : 0.02 * w, hiv .- lov) : vec_of(lr)
    (length(lov) == D && length(hiv) == D && length(lrv) == D) || error("maximize_acquisition_batch: lo, hi and lr must be scalars or of length $D")
    n = pending === nothing ? 0 : size(pending, 1)
    Xd = ROCArray{Float64}(permutedims(X0))
    Pd = n > 0 ? ROCArray{Float64}(permutedims(pending)) : nothing
    xb, ab, ib = ROCArray{Float64}(undef, D, q), ROCArray{Float64}(undef, q), ROCArray{Int64}(undef, q)
    GC.@preserve lov hiv lrv begin
        opts = Ref(PwAscentOpts(steps, 0, 0, beta1, beta2, eps, pointer(lov), pointer(hiv), pointer(lrv)))
        check(hm.ctx, ccall((:agp_svgp_acq_maximize_batch, libagp), Int32,
                            (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Float64, Int64, Ptr{Cvoid}, Int64, Int64,
                             Ref{PwAscentOpts}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                            hm.h, latent - 1, Ref(acq), n > 0 ? pointer(Pd) : C_NULL, D, n, pending_noise, q, pointer(Xd), D, R, opts,
                            pointer(xb), D, pointer(ab), pointer(ib)))
    end
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    Xb, a = permutedims(Array(xb)), Array(ab)
    return full ? (Xb, a, Array(ib) .+ 1) : (Xb, a)
end
# Joint batches ("ACQUISITION FUNCTIONS", paragraph "Joint batches"): Monte-Carlo q-EI (AcqDesc of EI) and q-UCB (of UCB) of q points under
# their posterior correlation, f_s = mu + L eps_s over the caller's base samples E (S x (q + n)); pending points are members of the
# joint sample that stay where they are.  Never run, like everything in this file.
# acquisition_joint(hm, acq, Xq, E; pending=nothing, grad=false, latent=1): alpha of the tuples Xq (n_sets x q x D), with grad=true
# (alpha, G n_sets x q x D) (agp_svgp_acquisition_joint)
function acquisition_joint(hm::HipModel{Float64}, acq::AcqDesc, Xq::AbstractArray{<:Real,3}, E::AbstractMatrix; pending=nothing,
                           grad::Bool=false, latent::Integer=1)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    nsets, q, D = size(Xq)
    n = pending === nothing ? 0 : size(pending, 1)
    S = size(E, 1)
    size(E, 2) == q + n || error("acquisition_joint: E must be S x (q + n)")
    Xd = ROCArray{Float64}(permutedims(Xq, (3, 2, 1)))        # column-major D x q x n_sets == [r][j][d]
    Ed = ROCArray{Float64}(permutedims(E))                    # column-major (q + n) x S == [s][k]
    Pd = n > 0 ? ROCArray{Float64}(permutedims(pending)) : nothing
    a = ROCArray{Float64}(undef, nsets)
    G = grad ? ROCArray{Float64}(undef, D, q, nsets) : nothing
    check(hm.ctx, ccall((:agp_svgp_acquisition_joint, libagp), Int32,
                        (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64,
                         Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                        hm.h, latent - 1, Ref(acq), n > 0 ? pointer(Pd) : C_NULL, D, n, q, pointer(Xd), D, nsets, pointer(Ed), q + n, S,
                        pointer(a), grad ? pointer(G) : C_NULL, D))
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    return grad ? (Array(a), permutedims(Array(G), (3, 2, 1))) : Array(a)
end
# maximize_acquisition_joint(hm, acq, X0, E, lo, hi; pending=nothing, steps=100, ...): the ascent of maximize_acquisition on the joint
# criterion, a start being a q-tuple (X0 is R x q x D) (agp_svgp_acq_maximize_joint).  Returns (X_best q x D, a_best); full=true adds
# idx (1-based), X (R x q x D) and A (R).
function maximize_acquisition_joint(hm::HipModel{Float64}, acq::AcqDesc, X0::AbstractArray{<:Real,3}, E::AbstractMatrix, lo, hi;
                                    pending=nothing, steps::Integer=100, lr=nothing, beta1::Real=0.9, beta2::Real=0.999,
                                    eps::Real=1e-8, latent::Integer=1, full::Bool=false)
    ensure_handle!(hm, max(hm.maxbatch, 1))
    R, q, D = size(X0)
    vec_of(v) = v isa Number ? fill(Float64(v), D) : collect(Float64, v)
    lov, hiv = vec_of(lo), vec_of(hi)
    lrv = lr === nothing ? map(w -> w == 0 ? 1.0 : 0.02 * w, hiv .- lov) : vec_of(lr)
    (length(lov) == D && length(hiv) == D && length(lrv) == D) || error("maximize_acquisition_joint: lo, hi and lr must be scalars or of length $D")
    n = pending === nothing ? 0 : size(pending, 1)
    S = size(E, 1)
    size(E, 2) == q + n || error("maximize_acquisition_joint: E must be S x (q + n)")
    Xd = ROCArray{Float64}(permutedims(X0, (3, 2, 1)))
    Ed = ROCArray{Float64}(permutedims(E))
    Pd = n > 0 ? ROCArray{Float64}(permutedims(pending)) : nothing
    X, A = ROCArray{Float64}(undef, D, q, R), ROCArray{Float64}(undef, R)
    xb, ab, ib = ROCArray{Float64}(undef, D, q), ROCArray{Float64}(undef, 1), ROCArray{Int64}(undef, 1)
    GC.@preserve lov hiv lrv begin
        opts = Ref(PwAscentOpts(steps, 0, 0, beta1, beta2, eps, pointer(lov), pointer(hiv), pointer(lrv)))
        check(hm.ctx, ccall((:agp_svgp_acq_maximize_joint, libagp), Int32,
                            (Ptr{Cvoid}, Int32, Ref{AcqDesc}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64,
                             Int64, Ref{PwAscentOpts}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                            hm.h, latent - 1, Ref(acq), n > 0 ? pointer(Pd) : C_NULL, D, n, q, pointer(Xd), D, R, pointer(Ed), q + n, S, opts,
                            full ? pointer(X) : C_NULL, D, full ? pointer(A) : C_NULL, pointer(xb), D, pointer(ab), pointer(ib)))
    end
    ccall((:agp_ctx_sync, libagp), Int32, (Ptr{Cvoid},), hm.ctx)
    check(hm.ctx, ccall((:agp_svgp_check_status, libagp), Int32, (Ptr{Cvoid},), hm.h))
    Xb, a_best = permutedims(Array(xb)), Array(ab)[1]
    full || return Xb, a_best
    return Xb, a_best, Array(ib)[1] + 1, permutedims(Array(X), (3, 2, 1)), Array(A)
end
acquisition(ho::HipOnlineModel, acq::AcqDesc, X::AbstractMatrix; kw...) = acquisition(ho.cur, acq, X; kw...)
maximize_acquisition(ho::HipOnlineModel, acq::AcqDesc, X0::AbstractMatrix, lo, hi; kw...) = maximize_acquisition(ho.cur, acq, X0, lo, hi; kw...)
acquisition_pending(ho::HipOnlineModel, acq::AcqDesc, X::AbstractMatrix, P::AbstractMatrix; kw...) = acquisition_pending(ho.cur, acq, X, P; kw...)
maximize_acquisition_batch(ho::HipOnlineModel, acq::AcqDesc, q::Integer, X0::AbstractMatrix, lo, hi; kw...) =
    maximize_acquisition_batch(ho.cur, acq, q, X0, lo, hi; kw...)
acquisition_joint(ho::HipOnlineModel, acq::AcqDesc, Xq::AbstractArray{<:Real,3}, E::AbstractMatrix; kw...) =
    acquisition_joint(ho.cur, acq, Xq, E; kw...)
maximize_acquisition_joint(ho::HipOnlineModel, acq::AcqDesc, X0::AbstractArray{<:Real,3}, E::AbstractMatrix, lo, hi; kw...) =
    maximize_acquisition_joint(ho.cur, acq, X0, E, lo, hi; kw...)

end # module
