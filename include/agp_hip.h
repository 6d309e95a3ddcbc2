/*
 * agp_hip.h -- C ABI of libagp_hip.so : MI355X (gfx950) engine for the SVGP + AnalyticVI/AnalyticSVI
 * hot path of AugmentedGaussianProcesses.jl (reference paths are relative to /root/reference).
 *
 * The reference has no FFI; this header is what a `ccall` shim binds (see INTEGRATION.md and
 * julia/AGPHip.jl).  Every entry point names the reference method(s) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross the boundary; every call returns agp_status.
 *   - all data pointers are DEVICE pointers unless the parameter name ends in `_host`.
 *   - element type T is double (AGP_F64) or float (AGP_F32), fixed per handle / per call.
 *   - inputs X, Z are POINT-MAJOR: point i occupies X[i*ldx .. i*ldx+D) (Julia `ColVecs` memory order;
 *     a `RowVecs` N x D column-major matrix is permuted once by the shim at upload).
 *   - m x m outputs are dense row-major with leading dimension m (all are symmetric or explicitly
 *     lower-triangular, so Julia column-major readers see the transpose == the same matrix / upper factor).
 *   - caller owns all data buffers; the library owns the opaque handles and their device workspaces.
 *   - work is enqueued asynchronously on the ctx stream; calls that return host scalars or a
 *     data-dependent status (refresh_K, elbo, check_status, ctx_sync) synchronise that stream.
 *
 * Environment (all the library reads; 18 variables, each read once per process unless said otherwise).  The first eight switch a
 * default path off for the FALLBACK that also exists on its own -- the GPU suite is run once with each of them, AGP_CHAIN_SPLIT both
 * ways (tools/suite_with_fallbacks.sh, profiles/r05_fallback_suites.txt); AGP_CHOL_GROUP, AGP_CHOL_LOOKAHEAD and the test hook
 * AGP_DAG_TEST_ABORT / AGP_DAG_TEST_FEED are exercised by tests of their own.  The A/B levers of earlier rounds are gone (docs/DESIGN_LOG.md has their numbers).
 *   AGP_CHOL_DAG=0|1          never / always factor with the one-launch tile task graph (default: up to 32 block columns, i.e. m <= 2048;
 *                             beyond, and after a lost dependency, plain launches per block column / blocked panels)
 *   AGP_CHAIN_SPLIT=0|1       the task graph as one kernel / as chain kernel + tile kernel (default: two kernels from 600 tiles,
 *                             except fp64 launches that carry the natural-gradient step as their prologue: those split only when
 *                             forced.  Round 6: the step's stream starts the tile kernel only when every chain workgroup of the
 *                             launch is resident -- DagSync::here, k_wait_here -- which removed the one way a split launch lost a
 *                             dependency on its own, docs/DESIGN_LOG.md sections 14 and 15)
 *   AGP_STEP_PROLOGUE=0       the natural-gradient step of a single-latent CAVI step as a kernel of its own (k_syrk_tn<SY_ETA2>)
 *                             instead of the prologue of the next step's task-graph launch
 *   AGP_STEP_EPILOGUE=0       the row statistics + local update as a kernel of their own instead of the launch's epilogue
 *   AGP_PF_INKERNEL=0         look-ahead stream handed over by events instead of polled words in signal memory
 *   AGP_KERNELMATRIX_VALU=1   kernel matrices by the direct-difference VALU kernel instead of the MFMA form (the path of D > 128)
 *   AGP_HYPER_GK_FUSED=0      hyper-gradient with kappa' H and K^-1 Sigma K^-1 (the form of handles without a prologue launch:
 *                             several latents, batch-sharded, online, stale-K) instead of the one product C (Sigma K^-1)
 *   AGP_SPLIT_MERGED=0        batch-parallel step: eta step and row statistics as kernels of their own (k_eta2_from_packed)
 *   AGP_GEMM_TALL=0|1         (round 6) never / wherever the shape allows: the kappa-type products on 128 x 64 C tiles (k_gemm_nt_tall) instead of
 *                             64 x 64 ones (default: fp64 products of more than 1100 64-tiles, i.e. C5's kappa GEMM)
 *   AGP_CHOL_GROUP=n          block columns per group of the blocked factorisation beyond the task graph (default 8; 1 = per column)
 *   AGP_CHOL_LOOKAHEAD=0      ... without its side stream
 *   AGP_DAG_TEST_ABORT=1      test hook: every task-graph launch of a CAVI step is treated as having lost a dependency (the in-stream
 *                             fallback k_chol_safe / k_safe_rowstats redoes it)
 *   AGP_DAG_TEST_FEED=1|2     test hook: how the chain workgroup of a task-graph launch takes in the two feeder tiles of the next block
 *                             column -- 1: every prefetched element of the diagonal tile counts as not yet visible and is re-loaded in
 *                             place (fp64 launches; fp32 has no such path) ; 2: the look at the feeders' flags always fails, so every
 *                             column takes the blocking fetch.  Same bits as the default on both (tests/test_gpu_chain_prefetch.py)
 *   AGP_DAG_TEST_OVERSUBSCRIBE=1  test hook (with AGP_DAG_TEST_ABORT=1): the fallback's grid is made too large to be resident at once, so
 *                             its grid barrier runs into its limit (8 s) and the step ends in status -3 / AGP_ERR_HIP instead of a hang
 *   AGP_SPLIT_OVERLAP=1       (read at every step) batch-parallel statistics travel in block-column groups next to the next
 *                             factorisation; see "multi-GPU" below
 *   AGP_FORCE_SPLIT=1         diagnostic: the batch-parallel step sequence with a one-rank communicator, its collective issued
 *   AGP_ALLOW_PARTIAL_SHARD=1 diagnostic: a latent-sharded multi-output handle may step without its communicator (bench.py c5, one GPU)
 *   AGP_RCCL_PATH=<file>      the librccl.so to bind when the process holds none (agp_comm_init)
 */
#ifndef AGP_HIP_H
#define AGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t agp_status;
enum {
  AGP_OK = 0,
  AGP_ERR_INVALID = 1,     /* bad argument */
  AGP_ERR_NOT_POSDEF = 2,  /* Julia PosDefException from cholesky(K + jitt*I)   src/gpblocks/latentgp.jl:206 */
  AGP_ERR_NEG_KTILDE = 3,  /* error("K~ has negative values")                   src/gpblocks/latentgp.jl:213 */
  AGP_ERR_BAD_BATCH = 4,   /* batch-size check                                  src/training/training.jl:27-29 */
  AGP_ERR_UNSUPPORTED = 5, /* implemented(likelihood, inference) == false       src/models/SVGP.jl:48-49 */
  AGP_ERR_LABELS = 6,      /* treat_labels! ArgumentError                       src/likelihood/classification.jl:36-44 */
  AGP_ERR_HIP = 7,         /* HIP runtime failure (message in agp_last_error) */
  AGP_ERR_NOMEM = 8
};

enum { AGP_F64 = 0, AGP_F32 = 1 };

/* KernelFunctions.jl kernels (call sites src/gpblocks/latentgp.jl:202-212): sigma2 * base(||s .* (x-y)||) */
enum { AGP_K_SQEXP = 0, AGP_K_MATERN52 = 1, AGP_K_MATERN32 = 2, AGP_K_EXPONENTIAL = 3 };

/* likelihoods with closed-form augmented updates (implemented(l, ::AnalyticVI) == true):
 * src/likelihood/{gaussian,logistic,studentt,logisticsoftmax,laplace,bayesiansvm,poisson,negativebinomial,heteroscedastic}.jl */
enum {
  AGP_LIK_GAUSSIAN = 0,
  AGP_LIK_LOGISTIC = 1,
  AGP_LIK_STUDENTT = 2,
  AGP_LIK_LOGISTICSOFTMAX = 3,
  AGP_LIK_MULTIOUTPUT = 4, /* MOSVGP handle: task likelihoods are installed by agp_svgp_set_multioutput */
  AGP_LIK_LAPLACE = 5,         /* LaplaceLikelihood(beta)            laplace.jl:17-25          p0 = beta */
  AGP_LIK_BAYESIANSVM = 6,     /* BayesianSVM()                      bayesiansvm.jl:19-23 */
  AGP_LIK_POISSON = 7,         /* PoissonLikelihood(lambda)          poisson.jl:16-24          p0 = initial lambda (state) */
  AGP_LIK_NEGBINOMIAL = 8,     /* NegBinomialLikelihood(r)           negativebinomial.jl:22-27 p0 = r */
  AGP_LIK_HETEROSCEDASTIC = 9, /* HeteroscedasticLikelihood(lambda)  heteroscedastic.jl:17-47  p0 = initial lambda (state);
                                  n_latent must be 2 (latent 0 = f, latent 1 = g) */
  AGP_LIK_SOFTMAX = 10         /* SoftMaxLikelihood(K)               softmax.jl:1-48           p0 unused, n_class = K as for
                                  LogisticSoftMax; no augmentation: AGP_FLAG_MC handles only ("MC INTEGRATION") */
};

/* ELBO variants: Appendix-A Q2 of SURVEY.md (src/likelihood/logistic.jl:82 uses dot(theta, mu)) */
enum { AGP_ELBO_CORRECTED = 0, AGP_ELBO_REFERENCE = 1 };

/* agp_svgp_desc.flags.
 * AGP_FLAG_STALE_K ("reference_compat_stale_K"): inside one train! the reference never recomputes
 * the Cholesky of K_ZZ after a hyper-parameter step -- compute_kernel_matrices (src/training/training.jl:187-208) only does
 * so while isHPupdated(inference), which update_hyperparameters! for sparse models never sets again (the call is commented
 * out, src/hyperparameter/autotuning.jl:41-46).  kappa = Knm / K then mixes the NEW kernel and Z (Knm, kdiag) with the OLD
 * factor, and natural_gradient! uses the old inv(K), until train! ends (compute_Ks, training.jl:107) or restarts without a
 * state.  The hyper-gradient itself is taken with fresh matrices (ELBO(m, x, y, mu0, ks, Zs, state) recomputes them,
 * src/functions/ELBO.jl:15-21).  With the flag a hyper step leaves the step-side matrices (L, inv(K), K\mu0) as they are and
 * only an explicit agp_svgp_refresh_K (what the host calls where train! starts and ends) recomputes them; without it
 * (default) K is refreshed before the next step. */
enum { AGP_FLAG_STALE_K = 1, AGP_FLAG_FULL = 2, AGP_FLAG_EXACT = 4, AGP_FLAG_SAMPLED = 8, AGP_FLAG_NUMERICAL = 16, AGP_FLAG_MC = 32 };
/* AGP_FLAG_FULL: the handle is the full (non-sparse) model VGP(X, y, kernel, likelihood, AnalyticVI())  src/models/VGP.jl:36-85 --
 * one latent of dimension N per n_latent(likelihood), kappa = I, prior K + jitt I on the training inputs themselves.  Create it with
 * m = max_batch = N, stochastic = 0, dtype AGP_F64 (other types: AGP_ERR_UNSUPPORTED); a Gaussian likelihood is refused with
 * AGP_ERR_UNSUPPORTED (VGP.jl:54-56).  agp_svgp_set_Z installs the training inputs X.  The entry points keep their meaning:
 *   cavi_step       idx = NULL, B = N (else AGP_ERR_BAD_BATCH); x is not read (the inputs are those of set_Z).  local_updates! on
 *                   mean_f = mu, var_f = diag Sigma (latentgp.jl:171-189), then eta1 = grad_E_mu + K \ mu0,
 *                   eta2 = -(Diagonal(grad_E_Sigma) + inv(K)/2) (analyticVI.jl:126-140); Sigma = -inv(eta2)/2, mu = Sigma eta1 by a
 *                   Cholesky of -2 eta2 (inference.jl:25-28).  rho is ignored.
 *   elbo            fresh_local = 0 (objective after a step) and 1 (fresh local variables), idx = NULL, B = N: expectation at
 *                   (mu, diag Sigma) - GaussianKL(mu, mu0, Sigma, K) - AugmentedKL (analyticVI.jl:255-274, KLdivergences.jl:11-18)
 *   get/set_state, get_matrix (AGP_MAT_KNM / AGP_MAT_KAPPA: AGP_ERR_UNSUPPORTED; AGP_VEC_KTILDE reads 0), refresh_K,
 *   set_prior_mean, get/set_lik_param, init_state, invalidate_data: as for SVGP, with Z = X
 *   hyper_step / hypergrad  gradient of the Gaussian KL w.r.t. the kernel parameters (autotuning.jl:49-85): the adjoint of K is
 *                   (K^-1 (Sigma + d d') K^-1 - K^-1) / 2, d = mu - mu0; X is never optimised (dZ / opt_Z: AGP_ERR_UNSUPPORTED)
 *   predict_f / predict_f_cov / predict_y / proba_y  the generic _predict_f with Zviews(m) = X (predictions.jl:25-50)
 * Refused with AGP_ERR_UNSUPPORTED, doing nothing: the phase entry points (step_local, lsm_*, step_stats, stats_ptr, step_global),
 * prefetch, batch sharding, every *_multi call, the online entry points, the latent-sharded multi-output calls (mo_shard,
 * mo_fbuf_ptr, mo_mix, mo_refresh_f, mo_predict_from_f); set_multioutput / get_A unless the likelihood is AGP_LIK_MULTIOUTPUT.
 *
 * AGP_FLAG_FULL with lik.kind = AGP_LIK_MULTIOUTPUT is MOVGP(X, y, kernel, likelihoods, AnalyticVI(), num_latent)
 * src/models/MOVGP.jl:46-126 -- n_latent = num_latent full latents on the training inputs (agp_svgp_set_Z installs X for every
 * latent; latent_offset = 0: all of them on one handle), mixed by A into one output per task.  agp_svgp_set_multioutput installs the
 * task likelihoods, A and the A optimiser exactly as for MOSVGP (a Gaussian task is allowed); targets are point-major
 * y[i * n_task + t].  What differs from VGP above:
 *   cavi_step       update_parameters!(::MOVGP) (training.jl:146-151): update_A! on mean_f_q = mu_q, var_f_q = diag Sigma_q of the
 *                   current posterior and the local variables of the step before, the local update of every task on the mixed
 *                   (sum_q A_tq mu_q, sum_q A_tq^2 diag Sigma_q), the mixed gradients per latent (analyticVI.jl:48-111), then
 *                   VGP's eta1 / eta2 for every latent at once
 *   elbo            sum_t expectation_t at the mixed (mean_f, var_f) - sum_q GaussianKL_q - sum_t AugmentedKL_t (analyticVI.jl:277-297)
 *   hyper_step / hypergrad  per latent as for VGP: only the Gaussian KL depends on a latent's kernel (autotuning.jl:48-84)
 *   predict_*       the multi-output _predict_f (predictions.jl:52-92) with Zviews(m) = X: out[n_task][n_t], means mixed by A,
 *                   variances and full covariances by A^2
 *   get_matrix      AGP_VEC_MEAN_F / AGP_VEC_VAR_F per latent (mu_q, diag Sigma_q as the last local phase saw them);
 *                   AGP_VEC_THETA / AGP_VEC_C count `latent` over the TASKS, as on every multi-output handle (below)
 * AGP_FLAG_EXACT with a multi-output likelihood: AGP_ERR_UNSUPPORTED. */
/* AGP_FLAG_EXACT (only together with AGP_FLAG_FULL): exact GP regression GP(X, y, kernel; noise, opt_noise) with Analytic()
 * inference  src/models/GP.jl:37-92, src/inference/analytic.jl:36-51.  Float64, n_latent = 1, a Gaussian likelihood (lik.p0 = sigma2,
 * lik.p1 = the ADAM rate of opt_noise or 0); anything else AGP_ERR_UNSUPPORTED.  elbo_mode AGP_ELBO_REFERENCE reproduces the
 * reference's three defects (G1 no kernel gradient, G2 ||alpha||_2 in the noise gradient, G3 y in place of y - mu0 in log p).
 *   cavi_step       idx = NULL, B = N, y = the targets (x is not read).  Sigma = K + sigma2 I (K + jitt I refreshed only when the
 *                   kernel moved), alpha = Sigma \ (y - mu0), log p; then, with opt_noise, one ADAM ascent step on log sigma2 with
 *                   the gradient (alpha' alpha - tr Sigma^-1) sigma2 / 2.  No host synchronisation.  rho is ignored.
 *   elbo            log p = -((y - mu0)' Sigma^-1 (y - mu0) + log det Sigma + N log 2 pi) / 2 of the stored posterior (GP.jl:87-92);
 *                   x, idx, B, rho and fresh_local are not read; y binds the targets when no step has been taken yet (a reloaded
 *                   model), else it is not read either
 *   refresh_K       compute_Ks + post_step!: K, then Sigma and alpha with the current sigma2 (what train! does where it ends)
 *   get_state       mu <- alpha, sigma <- Sigma; eta1 / eta2 must be NULL (else AGP_ERR_UNSUPPORTED).  set_state: AGP_ERR_UNSUPPORTED
 *   get_lik_param   sigma2 (synchronises)
 *   hyper_step / hypergrad / hyper_apply  d log p / d theta = tr((alpha alpha' - Sigma^-1) dK/dtheta) / 2 at the Sigma of the
 *                   last step.  The reference mode: hypergrad returns zeros, and neither hyper_step nor hyper_apply (whatever
 *                   gradient the caller supplies) steps the kernel or its optimiser state.  ExponentialKernel: AGP_ERR_UNSUPPORTED;
 *                   no dZ
 *   predict_f / predict_f_cov / predict_y / proba_y  mu* = K*n alpha, var* = k** + jitt - diag(K*n Sigma^-1 Kn*) (predictions.jl:6-23);
 *                   proba_y adds sigma2
 * Refused with AGP_ERR_UNSUPPORTED on top of AGP_FLAG_FULL's list: get_matrix, elbo_enqueue, elbo_terms. */
/* AGP_FLAG_SAMPLED (only together with AGP_FLAG_FULL, never with AGP_FLAG_EXACT): the Gibbs-sampled full model
 * MCGP(X, y, kernel, likelihood, GibbsSampling())  src/models/MCGP.jl:37-92, src/inference/gibbssampling.jl, src/training/sampling.jl.
 * Float64, one latent, likelihoods AGP_LIK_LOGISTIC, AGP_LIK_STUDENTT, AGP_LIK_NEGBINOMIAL (r an integer: Int(l.r),
 * negativebinomial.jl:87; otherwise AGP_ERR_INVALID).  A Gaussian likelihood is refused with the reference's message (MCGP.jl:54-56),
 * every other likelihood with AGP_ERR_UNSUPPORTED.  The handle's state is the current sample f (f = 0, Sigma = I at creation,
 * latentgp.jl:81-86) and the sweep counter t (0 at creation).  The chain is advanced by agp_svgp_gibbs_sample and read by
 * agp_svgp_predict_samples (below, "Gibbs sampling").  The other entry points:
 *   get_state       mu <- f, sigma <- Sigma = inv(2 Diagonal(grad_E_Sigma) + inv(K)) of the last sweep (I before the first);
 *                   eta1 / eta2 must be NULL (else AGP_ERR_UNSUPPORTED)
 *   set_state       eta1 = f installs the sample the chain continues from (a reloaded model), eta2 must be NULL
 *   get_matrix      AGP_VEC_THETA the local variables theta of the last sweep; AGP_VEC_C |f| as that sweep saw it (StudentT: the
 *                   InverseGamma draw omega = 1 / theta)
 *   set_Z, set_kernel, set_prior_mean, refresh_K, init_state, invalidate_data, get_lik_param: as for VGP.  The chain's state -- f,
 *                   Sigma of the last sweep and the sweep counter -- belongs to the model like VGP's posterior: init_state keeps it
 *                   (a new chain: a new handle, or set_state(f = 0) and agp_svgp_gibbs_counter(set = 1, 0))
 * Refused with AGP_ERR_UNSUPPORTED on top of AGP_FLAG_FULL's list: cavi_step, elbo, elbo_enqueue, elbo_terms (objective(::MCGP) =
 * NaN, MCGP.jl:91), hypergrad, hyper_step, hyper_apply, hyper_configure, hyper_rule (the reference never tunes an MCGP's kernel),
 * predict_f, predict_f_cov, predict_y, proba_y (they have no sample store: agp_svgp_predict_samples). */

/* matrices readable through agp_svgp_get_matrix (for parity tests and the shim's state export) */
enum {
  AGP_MAT_L = 0,      /* m x m lower Cholesky factor of K_ZZ + jitter I          (state.kernel_matrices.K) */
  AGP_MAT_KINV = 1,   /* m x m inv(K)                                             (analyticVI.jl:179) */
  AGP_MAT_KNM = 2,    /* B x m                                                    (latentgp.jl:210) */
  AGP_MAT_KAPPA = 3,  /* B x m                                                    (latentgp.jl:211) */
  AGP_VEC_KTILDE = 4, /* B                                                        (latentgp.jl:212) */
  AGP_VEC_MEAN_F = 5, /* B   kappa*mu   (value used by the last local update)     (latentgp.jl:179) */
  AGP_VEC_VAR_F = 6,  /* B                                                        (latentgp.jl:189) */
  AGP_VEC_THETA = 7,  /* B   local variable theta                                 (likelihood local_updates!) */
  AGP_VEC_C = 8,      /* B   local variable c (Laplace: b).  Heteroscedastic: latent 0 -> phi, latent 1 -> c.
                       *     Multi-output handles (MOSVGP, MOVGP, after set_multioutput): the local variables belong to the task
                       *     likelihoods, so for AGP_VEC_THETA / AGP_VEC_C `latent` counts the tasks, 0 <= latent < n_task */
  AGP_VEC_GAMMA = 9,  /* B   LogisticSoftMax gamma_k ; Poisson gamma ; Heteroscedastic: latent 0 -> gamma, latent 1 -> sigg */
  AGP_VEC_ALPHA = 10, /* B   LogisticSoftMax alpha (shared by all latents) */
  /* The two objects of the predictor ("PREDICTIVE GRADIENTS", "ACQUISITION FUNCTIONS"), as they stand after the predictor has been
   * brought up to date; every class that predicts, AGP_FLAG_EXACT included (there a = alpha, A = Sigma_y^-1); cap >= m.  The
   * predictor forms W = K*m A' with gemm_nt(Kstar, Apred): W_ij = sum_l k*_il Apred[j][l], rows of Apred as stored (A is symmetric
   * up to rounding; this is the index order the variance and its gradient use). */
  AGP_VEC_APRED = 11, /* m       a = K^-1 mu */
  AGP_MAT_APRED = 12  /* m x m   A = K^-1 - K^-1 Sigma K^-1, ldo >= m */
};

typedef struct agp_ctx agp_ctx;
typedef struct agp_svgp agp_svgp;

typedef struct {
  int32_t kind;                /* AGP_K_* */
  int32_t ard;                 /* 0: ScaleTransform(scale)   1: ARDTransform(ard_scales_host[0..D)) */
  double variance;             /* sigma2 of `sigma2 * k` (1 if none) */
  double scale;                /* s of ScaleTransform(s) ; with_lengthscale(k, l) == scale 1/l */
  const double* ard_scales_host; /* host pointer, length D, read at call time (only if ard) */
  /* Structure of the kernel OBJECT, which decides what the hyper-parameter step may touch: the reference differentiates the
   * kernel structurally (Zygote NamedTuple, autotuning.jl:99-118 -> update_kernel!, autotuning_utils.jl:47-67), so only
   * parameters that exist are stepped.  has_variance: the kernel is `sigma2 * k` (a ScaledKernel); has_transform: it is
   * `k o ScaleTransform / ARDTransform` (with_lengthscale included).  A bare SqExponentialKernel() has neither: its
   * hyper step leaves the kernel untouched (Z may still move).  Evaluation ignores both flags. */
  int32_t has_variance;
  int32_t has_transform;
} agp_kernel_desc;

typedef struct {
  int32_t kind;    /* AGP_LIK_* */
  int32_t n_class; /* LogisticSoftMax: K (= number of latent GPs); else 1 */
  double p0;       /* Gaussian: sigma2 ; StudentT: nu ; Laplace: beta ; NegBinomial: r ; Poisson / Heteroscedastic: lambda_0 */
  double p1;       /* StudentT: sigma ; Gaussian: learning rate of the optional noise optimiser -- GaussianLikelihood(sigma2;
                      opt_noise = ADAM(p1)), gaussian.jl:18-23,56-72; 0 = noise fixed.  With it sigma2 is STATE (stepped by every
                      local update in log space, read / set with agp_svgp_get/set_lik_param) */
} agp_lik_desc;

typedef struct {
  int32_t dtype;       /* AGP_F64 / AGP_F32  (SVGP(...; T=Float64) src/models/SVGP.jl:43) */
  int32_t n_latent;    /* latents held by THIS handle (latent-parallel ranks hold a slice) */
  int32_t latent_offset; /* global index of this handle's first latent (class index for LogisticSoftMax) */
  int32_t stochastic;  /* 0 AnalyticVI (Descent(1)) ; 1 AnalyticSVI (RobbinsMonro) analyticVI.jl:44-52 */
  int64_t m;           /* inducing points per latent */
  int64_t D;           /* input dimension */
  int64_t max_batch;   /* largest B ever passed to step / elbo */
  agp_lik_desc lik;
  double jitter;       /* <= 0 : reference default 1e-4 (f64) / 1e-3 (f32)  src/functions/utils.jl:8-9 */
  double rm_kappa;     /* RobbinsMonro kappa (0.51)  src/inference/optimisers.jl:6 */
  double rm_tau;       /* RobbinsMonro tau   (1)     */
  int32_t elbo_mode;   /* AGP_ELBO_* */
  int32_t flags;       /* AGP_FLAG_* */
} agp_svgp_desc;

/* ---- context ------------------------------------------------------------------------------------- */
int32_t agp_version(void);
/* hip_stream: a hipStream_t shared with the caller (AMDGPU.jl / torch) or NULL for the default stream */
agp_status agp_ctx_create(int32_t device, void* hip_stream, agp_ctx** out);
agp_status agp_ctx_destroy(agp_ctx* ctx);
agp_status agp_ctx_sync(agp_ctx* ctx);
/* Diagnostics (round 6): how many task-graph factorisation launches of this context lost a tile dependency and were re-run by their
 * in-stream fallback (k_chol_safe / k_safe_rowstats) since the context was created.  0 on a GPU this process has to itself -- a
 * non-zero count means steps that cost milliseconds instead of 0.3 and a trajectory that is correct to rounding but no longer the
 * bitwise one; bench.py prints it as `task_graph_fallbacks`.  Synchronises the context's stream. */
agp_status agp_ctx_task_graph_fallbacks(agp_ctx* ctx, int64_t* n_host);
const char* agp_last_error(agp_ctx* ctx);

/* ---- Layout: leading dimensions, padding, alignment (every entry point; pinned by tests/test_gpu_abi_layout.py) -----------
 *   - A leading dimension (ldx, ldy, ldo, lda, ldi, ldb, ldz, ldc, lds, ldza, ldf) counts ELEMENTS of T, not bytes, and must be at
 *     least the width of a row of its matrix: element (r, c) is base[r * ld + c], 0 <= c < width.  A smaller one is refused
 *     with AGP_ERR_INVALID before any buffer of the caller is read or written; the context / handle stays usable.
 *   - The ld - width elements behind every row, and everything in front of the first and behind the last element of a vector or
 *     matrix, are NEVER READ and NEVER WRITTEN -- they may hold NaN, or somebody else's data (a view into a larger array).
 *     Outputs are written in exactly rows x width elements, whatever the library pads to internally (tiles of 64).
 *   - A pointer needs the alignment of its element type only (8 bytes for double, 4 for float and int32, 8 for int64).  16-byte
 *     vector loads are used where base, leading dimension and width allow them, element loads elsewhere; the values are the same
 *     bit for bit either way, and do not depend on ld or on the base address.
 *   - Vectors (y, idx, mu0, mu, eta1, labels, counts, the B-sized outputs of get_matrix, predict outputs T[..][n_t]) are dense. */

/* ---- building blocks (unit parity) ---------------------------------------------------------------- */
/* kernelmatrix(k, X, Y) / kernelmatrix(k, X) (y == NULL -> symmetric)   src/gpblocks/latentgp.jl:206,210
 * idx (nullable, int64[n]) gathers rows of X: row i of the result uses X[idx[i]] (the view(X, minibatch) of
 * src/training/training.jl:54).  out is n x p row-major with leading dimension ldo >= p.
 * Symmetric form (y == NULL; p and ldy are not read): out is n x n, ldo >= n, out[i][j] = k(X[idx ? idx[i] : i], X[j]) -- idx
 * gathers the ROWS only, the columns are always x[0 .. n)  (kernelmatrix(k, X[idx]) needs a gathered copy of X).
 * Refused with AGP_ERR_INVALID: n <= 0, D <= 0, ldx < D, and with y: p <= 0, ldy < D, ldo < p; without y: ldo < n. */
agp_status agp_kernelmatrix(agp_ctx* ctx, int32_t dtype, const agp_kernel_desc* k, const void* x, int64_t n,
                            int64_t ldx, const int64_t* idx, const void* y, int64_t p, int64_t ldy, int64_t D,
                            void* out, int64_t ldo);
/* cholesky(A + jitter*I) in place, lower factor (strict upper zeroed).  *info_host = 0 ok, k>0: leading minor
 * k not positive definite (LAPACK potrf convention == Julia PosDefException.info).  src/gpblocks/latentgp.jl:206 */
agp_status agp_potrf_jitter(agp_ctx* ctx, int32_t dtype, void* a, int64_t lda, int64_t n, double jitter,
                            int32_t* info_host);
/* inv(A) for SPD A via Cholesky (inv(K::Cholesky) analyticVI.jl:179 ; -inv(eta2)/2 inference.jl:26) */
agp_status agp_spd_inverse(agp_ctx* ctx, int32_t dtype, const void* a, int64_t lda, int64_t n, void* ainv,
                           int64_t ldi, double* logdet_host, int32_t* info_host);
/* X = B / cholesky(A)  (Knm / K, two triangular solves in the reference, latentgp.jl:211); a is n x n (lda >= n), b and x are
 * r x n (ldb >= n, ldx >= n; r may exceed n) */
agp_status agp_solve_right_spd(agp_ctx* ctx, int32_t dtype, const void* a, int64_t lda, int64_t n, const void* b,
                               int64_t ldb, int64_t r, void* x, int64_t ldx, int32_t* info_host);
/* Accuracy (agp_potrf_jitter, agp_spd_inverse, agp_solve_right_spd).  With u the unit roundoff of T, the three are measured by
 *   eta = max_ij |A - L L'|_ij / sqrt(a_ii a_jj) (scaled backward error of the factor), phi = max_ij |L - L_exact|_ij / sqrt(a_ii),
 *   psi = max_ij |Y - A^-1|_ij / sqrt(A^-1_ii A^-1_jj) for the inverse Y, and chi = ||X - B A^-1||_max / ||B A^-1||_max for the
 *   solve, against a long-double reference (tests/_chol_ref.py, which holds the table measured on an MI355X).
 *   The factorisation multiplies by explicit inverses of its 32 x 32 diagonal blocks (L21 = A21 X11', panels P = T X') instead of
 *   substituting, which is conditionally stable: eta grows with the condition of those blocks -- 23 u ... 1.7e3 u on a squared-
 *   exponential K_ZZ + jitter I of condition 1e6 ... 2e10 in fp64 (LAPACK: 8 - 15 u), 6 - 32 u at condition 8e3 ... 2e5 in fp32.
 *   On a well-conditioned matrix eta is about sqrt(n) u / 2 on the diagonal (9 - 16 u at n = 136 ... 328, both types), because
 *   every S = D - L L' is accumulated on the tile in the MFMA accumulator; row and column scaling by powers of two changes
 *   nothing.  phi, psi and the log-determinant follow the conditioning as they do for LAPACK (within a factor 2 of a NumPy
 *   model of this arithmetic, which the tests hold them to with a factor 4).
 *   agp_solve_right_spd forms A^-1 = X' X and multiplies B by it: its residual ||X A - B|| grows with cond(A) u, where two
 *   triangular solves would stay at u -- callers that need a small residual at a large condition number should not rely on it.
 *   A pivot that is zero, negative or NaN is reported at its 1-based index (status AGP_ERR_NOT_POSDEF, *info_host = that index)
 *   by all three, on every driver; a NaN at A[i][k] is reported at max(i, k) + 1.  The context stays usable. */
/* ---- inducing-point selection (the step before the path) ----------------------------------------------------------------
 * `inducingpoints(KmeansAlg(m), X)` is how every reference example / test picks Z (test/testingtools.jl:66,
 * docs/examples/gpclassification.jl:47, docs/src/userguide.md:140-143).  The algorithm is third party and unvendored
 * (InducingPoints.jl kmeans_ip = AFK-MC2 seeding + Clustering.kmeans!(X, C; tol)); the deterministic part -- Lloyd
 * iterations from given seeds -- runs here, the random seeding stays with the caller (it needs the caller's RNG).
 *
 * agp_nearest_center: labels_out[i] = argmin_j ||x_i - c_j||^2 (ties -> smaller j), mind_out[i] = that squared distance
 *   (either output may be NULL); device pointers, row-major, x is n x D (ldx), centers m x D (ldc); D <= 128.
 * agp_kmeans: centers (in: seeds, out: result) ; Clustering.kmeans! control flow: assign, then repeat { centres <- cluster
 *   means (an emptied cluster keeps its centre) ; assign ; stop when |cost change| < tol } at most max_iter times.
 *   labels_out / counts_out: nullable device int32[n] / int32[m] of the final assignment: counts_out is the histogram of
 *   labels_out, also for max_iter = 0.  Synchronises.
 * Accuracy.  Distances are formed in T relative to the first centre, so the selection does not depend on where the data lies
 *   (unnormalised features are fine).  With u the unit roundoff of T, Dp = D rounded up to 16 and gamma_k = k u / (1 - k u), every
 *   point i has the budget B_i = 4 gamma_{Dp+4} (diam^2 + max_j ||x_i - c_j||^2), diam the largest distance between two centres:
 *   the centre labels_out[i] names is at most B_i farther (in squared distance) than the nearest one, mind_out[i] is within B_i of
 *   the nearest squared distance, and the cost within the sum of the B_i.  B_i holds differences only: it does not change when
 *   points and centres are translated.  Cluster means are sums in T of the raw coordinates (error relative to |x|, n_j terms), and
 *   the member counts are accumulated in T as well: an AGP_F32 cluster of more than 2^24 points is outside the contract.
 * Non-finite input.  A row of x with a NaN or an infinity gets a label in [0, m) (0 when all its distances are NaN) and a non-finite
 *   mind_out (NaN for a NaN; never 0); the other rows are unaffected.  agp_kmeans does not screen its input: such a row makes the
 *   centre it lands in, and the cost, non-finite. */
agp_status agp_nearest_center(agp_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t ldx, int64_t D,
                              const void* centers, int64_t ldc, int64_t m, int32_t* labels_out, void* mind_out);
agp_status agp_kmeans(agp_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t ldx, int64_t D, void* centers,
                      int64_t ldc, int64_t m, int32_t max_iter, double tol, int32_t* labels_out, int32_t* counts_out,
                      int32_t* iters_host, double* objective_host, int32_t* converged_host);
/* ---- kernel-aware selection: greedy conditional variance ------------------------------------------------------------------
 * `inducingpoints(ConditionalVariance(m, kernel), X)`.  k-means above clusters in raw input space and never sees the kernel; this
 * selection does.  It is the greedy MAP of a k-DPP (Chen, Zhang, Zhou, NeurIPS 2018) and the greedy conditional-variance selection
 * of Burt, Rasmussen, van der Wilk (JMLR 2020): a pivoted partial Cholesky factorisation of K_NN, which greedily reduces
 * tr(K_NN - K_NZ K_ZZ^-1 K_ZN), the trace term of the SVGP ELBO.
 *
 *   d_i = k(x_i, x_i) = variance.  For j = 0 .. m-1:
 *     p_j = argmax_i d_i                                     ties go to the SMALLER index, so p_0 = 0
 *     stop if d_{p_j} <= tol * variance                      (then n_selected = j)
 *     l_j = (k(X, x_{p_j}) - sum_{k<j} l_k * l_k[p_j]) / sqrt(d_{p_j}) ;  d <- d - l_j^2 ;  d_{p_j} <- 0: a chosen point has no
 *     residual left and is never chosen again.
 *
 * Float64 arithmetic throughout; x may be AGP_F32 (dtype) and is widened on load.  Kernel values are those of agp_kernelmatrix's
 * base function on the squared distance sum_d (s_d (x_d - z_d))^2, summed in ascending d.  All four kernels, a scale or ARD scales,
 * D <= 128.  The result is a function of the inputs alone (fixed summation orders, no atomics): two calls agree bit for bit, and
 * the first m' indices of a call with m > m' are those of a call with m'.
 *
 * x: n x D (ldx), device.  Outputs, all device except n_selected_host:
 *   idx_out     int64[m]             the chosen indices p_0 .. ; -1 behind n_selected
 *   z_out       m x D (ldz), dtype   the chosen rows, bit copies of x ; zero rows behind n_selected
 *   factor_out  nullable, n x m doubles (ldf >= m), row i = (l_0[i] .. l_{m-1}[i]) ; zero columns behind n_selected.
 *               factor_out[idx_out, :] is the lower Cholesky factor of K_ZZ.
 *   trace_out   nullable, double[m]  sum_i d_i after each step ; zero behind n_selected
 *   *n_selected_host                 how many points were chosen (m unless the stop rule fired)
 * Needs a workspace of 8 n m bytes for the factor (plus 8 n (D + 1)); AGP_ERR_NOMEM names the byte count when it cannot be had.
 * Refused with AGP_ERR_INVALID before anything is read or written: n <= 0, m <= 0, m > n, D <= 0, D > 128, ldx < D, ldz < D,
 * ldf < m (with factor_out), tol < 0 or NaN, a kernel descriptor with a kind outside 0..3, a variance or scale that is not positive
 * and finite, or ard without ard_scales_host.  Synchronises once, at the end; the Layout rules above hold. */
agp_status agp_greedy_variance(agp_ctx* ctx, int32_t dtype, const agp_kernel_desc* k, const void* x, int64_t n, int64_t ldx,
                               int64_t D, int64_t m, double tol, int64_t* idx_out, void* z_out, int64_t ldz,
                               void* factor_out, int64_t ldf, double* trace_out, int64_t* n_selected_host);
/* MFMA microbenchmark: TFLOP/s of back-to-back v_mfma_{f64,f32}_16x16x4 (roofline ceiling measurement) */
agp_status agp_mfma_peak(agp_ctx* ctx, int32_t dtype, double* tflops_host);

/* ---- SVGP model handle ---------------------------------------------------------------------------- */
/* SVGP(kernel, likelihood, AnalyticVI()/AnalyticSVI(B), Z)  src/models/SVGP.jl:33-80 ;
 * posterior init mu=0, Sigma=I, eta1=0, eta2=-I/2            src/gpblocks/posterior.jl:29-37 */
agp_status agp_svgp_create(agp_ctx* ctx, const agp_svgp_desc* desc, agp_svgp** out);
agp_status agp_svgp_destroy(agp_svgp* h);
/* per-latent kernel and inducing points (each latent owns a copy, latentgp.jl:63-68); marks K stale */
agp_status agp_svgp_set_kernel(agp_svgp* h, int32_t latent, const agp_kernel_desc* k);
agp_status agp_svgp_set_Z(agp_svgp* h, int32_t latent, const void* z, int64_t ldz);
agp_status agp_svgp_get_Z(agp_svgp* h, int32_t latent, void* z, int64_t ldz);
/* prior mean values at Z (NULL == ZeroMean, src/mean/zeromean.jl:17) */
agp_status agp_svgp_set_prior_mean(agp_svgp* h, int32_t latent, const void* mu0);
/* compute_K for every latent with a stale K: K = k(Z,Z)+jitt I = L L', inv(K)   latentgp.jl:205-207.
 * Synchronises; AGP_ERR_NOT_POSDEF if any factorisation failed. */
agp_status agp_svgp_refresh_K(agp_svgp* h);
/* RobbinsMonro counters (state_eta1/state_eta2, src/training/states.jl:63-70); n starts at 1 */
agp_status agp_svgp_set_opt_state(agp_svgp* h, int64_t n);
agp_status agp_svgp_get_opt_state(agp_svgp* h, int64_t* n_host);

/* update_parameters!(model::SVGP, state, x, y)  src/training/training.jl:140-144 : one CAVI step on the
 * minibatch X[idx[0..B)] for all latents of this handle.
 *   y   : T[N] (+-1 labels / real targets) ; LogisticSoftMax: int32[N] 0-based class index
 *   idx : int64[B] device, or NULL for rows 0..B-1 (full batch)
 *   rho : N / B   (training.jl:30)
 * Asynchronous; data-dependent failures (K~ <= 0, non-SPD -2*eta2) are latched and reported by
 * agp_svgp_check_status / the next synchronising call.
 * Scheduling note (round 3, invisible through the ABI): for a single-latent handle in a training loop (look-ahead or full batch,
 * up to 16 block columns of 64) the natural-gradient step of this minibatch (natural_gradient! + global_update!,
 * analyticVI.jl:143-180, 229-246) is not enqueued by this call but rides as the PROLOGUE of the NEXT step's factorisation launch;
 * every other entry point of the handle first takes a pending step with the stand-alone kernel, so eta, Sigma, the ELBO, the
 * hyper-gradient and predictions always see the completed step (AGP_STEP_PROLOGUE=0 switches the scheduling off).  x, y, idx of a
 * step are not read again after the call that follows it. */
agp_status agp_svgp_cavi_step(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx,
                              int64_t B, double rho);
/* Diagnostics of the scheduling described above: number of agp_svgp_cavi_step calls on this handle, and how many of them had their
 * natural-gradient part taken as the prologue of the following step's factorisation launch (the rest took it with the stand-alone
 * kernel).  bench.py reads them to decide what the dominant launch contained.  Host counters, no synchronisation. */
agp_status agp_svgp_step_counters(agp_svgp* h, int64_t* n_steps_host, int64_t* n_prologue_host);
/* ... and of the hyper-parameter iteration (round 4): number of hyper-gradient evaluations on this handle, and how many of them
 * formed G_K from ONE m^3 product -- C (Sigma K^-1) with C = kappa' diag(w) kappa + K^-1 / 4 left behind by the prologue of the
 * factorisation launch -- instead of kappa' H and K^-1 Sigma K^-1 (update_hyperparameters!, autotuning.jl:86-140).  Host counters. */
agp_status agp_svgp_hyper_counters(agp_svgp* h, int64_t* n_grad_host, int64_t* n_gk_fused_host);
/* The same step in phases, for multi-GPU runs:
 *   step_local  : compute_kappa + mean_f/var_f (+ c_k for LogisticSoftMax)   latentgp.jl:209-215,171-189
 *   lsm_*       : LogisticSoftMax cross-latent fixed point, logisticsoftmax.jl:65-72:
 *                 lsm_gamma writes gamma_k for local latents and their sum into the `gsum` buffer (T[B]);
 *                 the caller all-reduces gsum across latent-parallel ranks; lsm_alpha sets alpha = 1 + gsum.
 *                 (called twice, as the reference loops twice)
 *   step_stats  : theta, grad_E_mu, grad_E_Sigma and the batch statistics
 *                 stats = [ kappa'(rho g1) (mp) | rho kappa' diag(g2) kappa, lower 64x64 tiles packed block column by block
 *                 column: tile (i, j <= i) of the nt x nt grid (nt = mp / 64) at offset mp + (j nt - j(j-1)/2 + i - j) * 4096,
 *                 row-major inside the tile ] per latent
 *                 -- the buffer a batch-parallel run all-reduces (analyticVI.jl:168,179)
 *   step_global : natural-gradient step + (mu, Sigma) refresh      analyticVI.jl:229-246, inference.jl:25-28 */
agp_status agp_svgp_step_local(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx,
                               int64_t B, double rho);
/* Hyper-parameter / inducing-point step: update_hyperparameters!(m, state, x, y)  src/hyperparameter/autotuning.jl:86-140
 * = reverse mode of ELBO(model, x, y, mu0, kernels, Zs, state) (src/functions/ELBO.jl:15-21; (mu, Sigma, local variables)
 * fixed, AugmentedKL ignored) w.r.t. the kernel parameters (variance, ScaleTransform / ARDTransform scales) and Z,
 * hand-derived instead of Zygote, on the minibatch of the LAST cavi_step; then ADAM ascent with the positive kernel
 * parameters stepped in log space (update_kernel!, autotuning_utils.jl:63-67) and Z directly (update_Z!, :70-76).
 * K is marked stale and refreshed by the next step (the reference leaves it stale inside train!).
 *   hyper_configure : optimiser=ADAM(kernel_eta) / Zoptimiser=ADAM(z_eta) of SVGP(...)  (SVGP.jl:39-42); 0 disables
 *   hypergrad       : the gradient only (parity): dscale_host[D] per input dimension (a ScaleTransform's single
 *                     parameter receives their sum), dZ device T[m][D] (nullable)
 *   get_kernel      : current variance and per-dimension scales
 * Limits of hypergrad / hyper_step (sparse and AGP_FLAG_FULL handles alike): the input dimension D must be at most 64 (the backward
 * pass through the kernel matrix stages 32 dimensions at a time and keeps two such chunks per tile: HB_MAXD, agp_hyper.h), and the
 * kernel must be SqExponential, Matern32 or Matern52 (the ExponentialKernel is not differentiable at zero distance).  Otherwise
 * both return AGP_ERR_UNSUPPORTED with the reason in agp_last_error, before anything is launched: dvariance_host, dscale_host and
 * dZ are not touched, and the handle goes on taking steps and predicting.  Steps, ELBO and
 * predictions themselves have no such limit on D.  Pinned at D = 1, 31, 32, 33, 64 and 65 by tests/test_gpu_hyper_edges.py.
 * agp_svgp_predict_f_grad ("PREDICTIVE GRADIENTS" below) differentiates the same kernels with respect to the input and has the same
 * two limits, refused the same way. */
agp_status agp_svgp_hyper_configure(agp_svgp* h, int32_t opt_kernel, double kernel_eta, int32_t opt_Z, double z_eta,
                                    double adam_b1, double adam_b2, double adam_eps);
/*   hyper_rule      : which Optimisers.jl rule `optimiser` / `Zoptimiser` are (the reference hands whatever rule it is given to
 *                     Optimisers.apply, src/hyperparameter/autotuning_utils.jl:47-82): ADAM (default; eta and the moments from
 *                     hyper_configure), Descent(eta): dx' = eta dx, Momentum(eta, rho): vel = rho vel + eta dx, dx' = vel.
 *                     The optimiser state exported by agp_svgp_hyper_opt_state holds the velocity in the first-moment slot. */
enum { AGP_OPT_ADAM = 0, AGP_OPT_DESCENT = 1, AGP_OPT_MOMENTUM = 2 };
agp_status agp_svgp_hyper_rule(agp_svgp* h, int32_t kernel_rule, double kernel_rho, int32_t z_rule, double z_rho);
agp_status agp_svgp_hypergrad(agp_svgp* h, int32_t latent, double* dvariance_host, double* dscale_host, void* dZ);
agp_status agp_svgp_hyper_step(agp_svgp* h);
/* the optimiser half of hyper_step with a caller-supplied gradient in the layout of agp_svgp_hypergrad (dZ: device m x D,
 * nullable).  hypergrad + hyper_apply == hyper_step; in between a multi-GPU driver can sum the gradient over latents and
 * all-reduce it over ranks (tied-Z mode: one kernel and one Z shared by all latents, BASELINE.json config 4). */
agp_status agp_svgp_hyper_apply(agp_svgp* h, int32_t latent, const double* dvariance_host, const double* dscale_host,
                                const void* dZ);
agp_status agp_svgp_get_kernel(agp_svgp* h, int32_t latent, double* variance_host, double* scales_host);
/* ADAM moments of a latent's kernel-parameter optimiser (hyperopt_state.state_k of the reference's state): host arrays of
 * 1 + D doubles (entry 0 variance, then scales; a ScaleTransform uses entry 1), set = 0 reads, set = 1 writes.  Lets a
 * streaming model (OnlineSVGP: a new handle per batch) and a resumed run continue the optimiser instead of restarting it. */
agp_status agp_svgp_hyper_opt_state(agp_svgp* h, int32_t latent, int32_t set, double* k_m_host, double* k_v_host,
                                    int32_t* k_step_host);
/* Multi-output model  MOSVGP(kernel, likelihoods, inference, Zs; Aoptimiser)  src/models/MOSVGP.jl:33-115 on a handle
 * created with lik.kind = AGP_LIK_MULTIOUTPUT: the handle's n_latent latent GPs are mixed into n_task outputs
 * f_t = sum_q A[t][q] f_q (mean_f / var_f / grad mixing: src/models/single_and_multi_output_utils.jl:24-84).
 *   liks_host : n_task likelihoods (Gaussian / Logistic / StudentT: one latent function per task)
 *   A_host    : n_task x n_latent row-major mixing weights (rows normalised, MOSVGP.jl:101-104)
 *   y passed to the step / ELBO calls is then point-major T[N][n_task] (task t's target of point i at y[i*n_task + t])
 *   adam_eta > 0 enables update_A! (ADAM ascent + projection on the unit sphere, lines 87-118); <= 0: Aoptimiser=false
 * predict_f / predict_y / proba_y outputs become T[n_task][n_t] (Bernoulli tasks: predict_y -> 1.0 / 0.0). */
agp_status agp_svgp_set_multioutput(agp_svgp* h, int32_t n_task, const agp_lik_desc* liks_host, const double* A_host,
                                    double adam_eta, double adam_b1, double adam_b2, double adam_eps);
agp_status agp_svgp_get_A(agp_svgp* h, double* A_host);
/* Latent-sharded multi-output model (C5 = 16 latents over 8 GPUs): every rank's handle owns the latents
 * [desc.latent_offset, desc.latent_offset + desc.n_latent) of q_total.  Call agp_svgp_mo_shard BEFORE set_multioutput; A_host /
 * get_A are then n_task x q_total (replicated on every rank, update_A! runs redundantly and stays bit-identical).  The mixing
 * (single_and_multi_output_utils.jl:24-84) needs every latent's (mean_f, var_f) on the minibatch; they travel through one
 * exchange buffer T[2][q_total][Bp] (mo_fbuf_ptr; own rows filled, the others zero, so an all-reduce(sum) over the ranks is
 * the all-gather).  One training step:
 *     step_local -> all-reduce(fbuf) -> mo_mix -> step_stats -> step_global
 * ELBO (fresh_local = 0) and hypergrad / hyper_step need the mixed means under the UPDATED posterior:
 *     mo_refresh_f -> all-reduce(fbuf) -> elbo / hypergrad     (elbo returns this rank's share: sum the scalars over ranks)
 * predict_f returns this rank's PARTIAL mix sum_{q owned} A[t][q]^p f_q: all-reduce it; predict_y / proba_y are then
 * finished in place by mo_predict_from_f (mode 0: out0 = mixed mean_f -> predict_y ; mode 1: out0, out1 = mixed mean_f,
 * var_f -> proba_y's two outputs; the Gauss-Hermite rule is only read for Bernoulli / NegBinomial tasks in mode 1). */
agp_status agp_svgp_mo_shard(agp_svgp* h, int32_t q_total);
agp_status agp_svgp_mo_fbuf_ptr(agp_svgp* h, void** ptr, int64_t* count);
agp_status agp_svgp_mo_mix(agp_svgp* h);
agp_status agp_svgp_mo_refresh_f(agp_svgp* h);
agp_status agp_svgp_mo_predict_from_f(agp_svgp* h, int64_t n_t, int32_t mode, void* out0, void* out1,
                                      const double* gh_nodes_host, const double* gh_weights_host, int32_t n_nodes);
/* Optional look-ahead: compute Knm / kappa of the NEXT minibatch (compute_kappa, latentgp.jl:209-215) on a second,
 * library-owned stream so it overlaps the current step's latency-bound factorisation.  The next cavi_step /
 * step_local called with the same (x, ldx, idx, B) adopts the result; any other call simply ignores it.
 * CONTRACT: the look-ahead is recognised by POINTER IDENTITY of (x, ldx, idx, B).  Between this call and the step that adopts it
 * the index buffer must stay allocated AND unchanged (the step gathers nothing again: it takes the rows the look-ahead read), and so
 * must the rows of x it names.  A host that refills one index buffer per iteration therefore either alternates between two
 * buffers or calls agp_svgp_invalidate_data (which also drops a pending look-ahead) after refilling.  Kernel / Z / state changes
 * (set_kernel, set_Z, hyper steps, refresh_K) drop it by themselves. */
agp_status agp_svgp_prefetch(agp_svgp* h, const void* x, int64_t ldx, const int64_t* idx, int64_t B);
agp_status agp_svgp_lsm_gamma(agp_svgp* h);
agp_status agp_svgp_lsm_alpha(agp_svgp* h);
agp_status agp_svgp_lsm_gsum_ptr(agp_svgp* h, void** ptr, int64_t* count);
agp_status agp_svgp_step_stats(agp_svgp* h);
agp_status agp_svgp_stats_ptr(agp_svgp* h, void** ptr, int64_t* count);
agp_status agp_svgp_step_global(agp_svgp* h);
/* Measurement hook (bench.py roofline): when enabled, every factorisation sequence of a CAVI step (the launches of
 * the dominant kernel: k_chol_dag, or the launches of k_chol_step) is bracketed by HIP events recorded on the ctx stream.  timing_read
 * synchronises, returns the number of bracketed kernel launches and their summed duration, and resets.
 * on = 1: every sequence; on = n > 1: every n-th sequence (the two event records cost a C2 step about 16 us). */
agp_status agp_svgp_timing_enable(agp_svgp* h, int32_t on);
agp_status agp_svgp_timing_read(agp_svgp* h, int64_t* n_launches_host, double* total_ms_host);
/* returns and clears the latched asynchronous failure (synchronises) */
agp_status agp_svgp_check_status(agp_svgp* h);

/* ELBO(model, state, y)  src/inference/analyticVI.jl:255-274
 *   fresh_local = 0 : on the kernel matrices and local variables left by the last cavi_step (x, y, idx, B
 *                     must be that step's) -- `objective(model, state, y)` of training.jl:76
 *   fresh_local = 1 : external ELBO(model, X, y) of src/functions/ELBO.jl:32-47 : recompute kappa on this
 *                     batch, re-initialise local variables, one local update, then the ELBO; rho explicit.
 *                     Round 6: when the SAME batch (pointer identity of x and idx, same B / ldx) is evaluated again with no training
 *                     step, kernel / Z change or agp_svgp_invalidate_data in between -- a handle used for monitoring only -- K_nm and
 *                     kappa of that batch are kept, like the full-batch kappa cache of the step. */
agp_status agp_svgp_elbo(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                         double rho, int32_t fresh_local, double* elbo_host);
/* The same evaluation WITHOUT a host round trip (convergence monitoring: `objective(model, state, y)` every few iterations of
 * train!, training.jl:71-90, evaluated while the next iterations are already enqueued).  enqueue puts the evaluation into the
 * stream and returns a ticket (up to 8 in flight); the value lands in mapped host memory behind an event.  fetch returns it:
 * wait = 1 blocks until it is there; wait = 0 only reports (*ready = 0 / 1).  A fetched ticket is closed.  Models whose ELBO has
 * host-side pieces (several latents, multi-output, streaming prior, AGP_FLAG_STALE_K) are evaluated synchronously inside enqueue.
 * agp_svgp_elbo_terms keeps referring to the last SYNCHRONOUS evaluation. */
agp_status agp_svgp_elbo_enqueue(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                                 double rho, int32_t fresh_local, int32_t* ticket);
agp_status agp_svgp_elbo_fetch(agp_svgp* h, int32_t ticket, int32_t wait, double* elbo_host, int32_t* ready);
/* the three terms of the last agp_svgp_elbo call, ELBO = rho * terms[0] - terms[1] - rho * terms[2]: unscaled data term
 * (expec_loglikelihood), Gaussian KL (+ extraKL), unscaled augmented KL.  A batch-parallel driver sums terms 0 and 2 over the
 * minibatch shards and counts the (replicated) Gaussian KL once. */
agp_status agp_svgp_elbo_terms(agp_svgp* h, double* terms_host);

/* ---- STREAMED ELBO (the full-data objective of an AnalyticSVI run, over any number of points) ---------------------------------
 * External ELBO(model, X, y) (src/functions/ELBO.jl:28-47) over ANY number of points, streamed: fresh local variables,
 * one local update, rho explicit.  No n x m object, no per-point vector of length n; workspace independent of n.
 *
 * Meaning.  The value is what agp_svgp_elbo(..., fresh_local = 1) returns for the same points in one batch.  terms_host (nullable,
 * double[3]) = (unscaled data term, Gaussian KL, unscaled augmented KL), ELBO = rho * t0 - t1 - rho * t2, as agp_svgp_elbo_terms
 * defines them.  idx is nullable; when given, the rows of x and y are read at idx[i] (device memory, n entries).  n is NOT bounded
 * by max_batch; n = 0 is AGP_ERR_BAD_BATCH.  x NULL, y NULL, elbo_host NULL, ldx < D or rho <= 0 are AGP_ERR_INVALID.  Layout: the
 * "Layout" section above (ldx in elements, >= D, padding never read); y as agp_svgp_cavi_step takes it (T[n], int32 class indices
 * for LogisticSoftMax).
 *
 * How.  Chunks of 4096 points go through the predictor's kernels (mean_f = k_* K^-1 mu, var_f = k_** + jitter - rowdot(k_* A, k_*),
 * A = K^-1 - K^-1 Sigma K^-1, algebraically K~ + diag(kappa Sigma kappa')); one kernel forms the local variables of each point in
 * registers and leaves one pair of partial sums per 256 points; ONE fixed-order reduction adds all partials after the last chunk.
 * No floating-point atomics: two calls on the same inputs return the same bits.  The only allocation that grows with n is the
 * partial sums, 16 bytes per 256 points.
 *
 * Once-per-evaluation terms of the reference are counted ONCE for the whole stream and read from global point 0 (the first chunk's
 * first point), exactly as the one-batch call does: LogisticSoftMax log(beta[0]) (with the GammaEntropy sums per point), and in
 * AGP_ELBO_REFERENCE mode the Laplace GIGEntropy's scalar-iteration terms of point i == 0.
 *
 * No side effects.  The call completes a pending natural-gradient step first, as every entry point does.  After that it leaves
 * unchanged: the posterior, the local variables of the last step, the kappa / K_nm caches and their validity flags, the look-ahead,
 * agp_svgp_elbo_terms (which keeps referring to the last agp_svgp_elbo) and the status word (nothing is latched).  It uses the
 * predictor's workspace and caches, like agp_svgp_predict_f.
 *
 * Failure.  If a point's var_f is not > 0, or a moment is not finite, the call returns AGP_ERR_NEG_KTILDE and agp_last_error
 * carries the index (position in the stream) of the FIRST such point; a LogisticSoftMax class index outside [0, n_class) returns
 * AGP_ERR_LABELS in the same way.  elbo_host and terms_host stay untouched.  The call synchronises once per latent, at the end
 * (the Gaussian KL's scalars; the data terms and the failure words ride on the first).
 *
 * Accepted: sparse AnalyticVI / AnalyticSVI handles, AGP_F64 and AGP_F32; Gaussian with fixed noise, Logistic, StudentT, Laplace,
 * BayesianSVM, NegBinomial, LogisticSoftMax (all K latents on the handle); both elbo_modes, every kernel and transform, any D,
 * non-zero prior mean.
 * Refused with AGP_ERR_UNSUPPORTED, by name in agp_last_error, before anything is launched: Poisson and Heteroscedastic (lambda is
 * re-estimated from sums over the whole batch: a second pass); Gaussian with opt_noise (its fresh ELBO steps the noise);
 * AGP_LIK_MULTIOUTPUT; AGP_FLAG_FULL, AGP_FLAG_EXACT, AGP_FLAG_SAMPLED, AGP_FLAG_NUMERICAL and AGP_FLAG_MC handles; online handles
 * (streaming prior); AGP_FLAG_STALE_K; latent-sharded and batch-sharded handles. */
agp_status agp_svgp_elbo_stream(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t n,
                                double rho, double* elbo_host, double* terms_host /* nullable, double[3] */);

/* ---- LOG PREDICTIVE DENSITY (held-out log-likelihood / NLPD, over any number of test points) ------------------------------------
 * sum_i lpd_i, lpd_i = log p(y_i | x_i, model) = log int p(y_i | f) N(f; mu_i, var_i) df, where (mu_i, var_i) are exactly what
 * agp_svgp_predict_f with variances returns for the handle and p(y | f) is the reference's point likelihood.  Streamed in chunks
 * of 4096 points through the handle's own predictor; the sum comes back in double (sum_host), the vector optionally (lpd_out,
 * nullable, device T[n], dense).  Layout: the "Layout" section above (ldx in elements, >= D, padding never read); y as
 * agp_svgp_cavi_step takes it (T[n]; int32 class indices for LogisticSoftMax / SoftMax).
 *
 * The rule per likelihood.
 *   Gaussian      closed form, log N(y; mu, var + sigma2) with the handle's CURRENT noise (the opt_noise state included).
 *   Laplace(beta) closed form (Gauss-Hermite converges slowly across the kink): with d = y - mu,
 *                 p = (1 / 4 beta) [T(d) + T(-d)], T(d) = exp(var / 2 beta^2 - d / beta) erfc((var / beta - d) / sqrt(2 var)),
 *                 formed in logs (erfc below a = 0, exp(-d^2 / 2 var) erfcx(a) above) and combined with logaddexp: finite for
 *                 |d| = 50 at var = 1e-3 and at var = 30.
 *   Logistic, BayesianSVM, StudentT, Poisson, NegBinomial
 *                 the n-node Gauss-Hermite sum in f-space with the caller's nodes and weights, the reference's predictive rule
 *                 (predictions.jl:4, classification.jl:14-26; the nodes agp_svgp_proba_y takes: x_j = sqrt(2) t_j, w_j = omega_j /
 *                 sqrt(pi)), 1 <= n_nodes <= 4096: lpd = log sum_j w_j p(y | mu + sqrt(var) x_j), formed as a log-sum-exp of
 *                 log w_j + log p with every log p in its overflow-safe form (mu = -800 y at var = 1e-2 gives about -800 where the
 *                 direct sum gives -inf).  Poisson uses the handle's current lambda.  StudentT takes the reference's density AS
 *                 WRITTEN (studentt.jl:43-46): Gamma(alpha) / (sqrt(nu pi) Gamma(nu / 2)) (1 + ((y - f) / sigma)^2)^-alpha, alpha =
 *                 (nu + 1) / 2 -- the normalised t with nu degrees of freedom and scale sigma / sqrt(nu), multiplied by sigma /
 *                 sqrt(nu) (the constant the quadrature inference uses).
 *                 Accuracy: the f-space rule degrades when the predictive spread sqrt(var) far exceeds the likelihood's width;
 *                 DESIGN.md section 9m has the measured table.
 *   LogisticSoftMax / SoftMax
 *                 the handle's own proba_y rule, the link applied to the means (multiclass.jl:96-117): lpd = log sigma(mu_y) -
 *                 log sum_k sigma(mu_k), resp. mu_y - logsumexp(mu), formed in logs.  The variances are only checked.
 *
 * How.  Quadrature kinds: a 16-lane group per point, node j on lane j mod 16, a running (max, scaled sum) pair per lane, merged by
 * a fixed shuffle tree; the others one lane per point.  Double accumulation for both dtypes.  One partial sum per workgroup, ONE
 * fixed-order reduction after the last chunk, no floating-point atomics: two calls on the same inputs return the same bits, sum and
 * vector.  The partial sums are the only allocation that grows with n (at most 1 byte per point); the rest is chunk-sized and kept
 * on the handle.  The nodes live in a device buffer that is uploaded only when the caller's rule changes.
 *
 * No side effects.  The call completes a pending natural-gradient step first, as every entry point does; after that it uses the
 * predictor's workspace and caches, like agp_svgp_predict_f, and buffers of its own -- the posterior, step buffers, local variables,
 * caches, agp_svgp_elbo_terms and the status word stay bitwise unchanged.  It synchronises once, at the end (and once more before
 * it uploads a rule that differs from the last call's).
 *
 * Failure.  A point whose var_f is not > 0, or a moment that is not finite: AGP_ERR_NEG_KTILDE.  A class index outside [0, K), a
 * Poisson / NegBinomial target that is not a non-negative integer, a Logistic / BayesianSVM label that is not +-1:
 * AGP_ERR_LABELS.  agp_last_error names the FIRST such position of the stream.  sum_host is then untouched, the contents of lpd_out
 * are unspecified, nothing is latched on the handle.  n = 0 succeeds with sum 0.  n < 0, sum_host NULL, x / y NULL, ldx < D, missing
 * nodes for a quadrature kind, n_nodes outside [1, 4096], negative or non-finite weights: AGP_ERR_INVALID.
 *
 * Accepted: every handle whose agp_svgp_predict_f works -- sparse AnalyticVI / AnalyticSVI (AGP_F64 and AGP_F32), online,
 * AGP_FLAG_STALE_K, AGP_FLAG_FULL, AGP_FLAG_EXACT, AGP_FLAG_NUMERICAL with or without AGP_FLAG_MC (their (mu, Sigma) are always valid
 * for prediction).  Refused with AGP_ERR_UNSUPPORTED, by name in agp_last_error, before anything is launched: Heteroscedastic (two
 * latents, a nested integral: a follow-up); AGP_LIK_MULTIOUTPUT; AGP_FLAG_SAMPLED; latent-sharded and batch-sharded handles. */
agp_status agp_svgp_lpd_stream(agp_svgp* h, const void* xt, int64_t ldx, const void* y, int64_t n, const double* gh_nodes_host,
                               const double* gh_weights_host, int32_t n_nodes, double* sum_host,
                               void* lpd_out /* nullable, device T[n] */);
/* The point-wise kernel of the above on given moments, outside any model (what agp_quad_expectations is to the quadrature
 * inference): lpd_out[i] (device T[n]) from y[i] and mu / var (device T[n]; T[n_class][ld] for the multi-class kinds, ld >= n the
 * latent stride).  dtype AGP_F64 / AGP_F32.  The nodes may be NULL for the closed-form and multi-class kinds.  Gaussian sigma2,
 * Laplace beta, NegBinomial r and Poisson lambda are lik->p0; StudentT (nu, sigma) = (p0, p1); n_class = K.  Failures as above (the
 * position is the index i); n = 0 is a successful no-op.  Synchronises the context's stream. */
agp_status agp_log_predictive(agp_ctx* ctx, int32_t dtype, const agp_lik_desc* lik, const void* y, const void* mu, const void* var,
                              int64_t n, int64_t ld /* latent stride, >= n */, const double* gh_nodes_host,
                              const double* gh_weights_host, int32_t n_nodes, void* lpd_out);
/* batch-parallel run: this handle sees shard `rank` of `world` of every minibatch.  Changes the ELBO -- the reference's
 * once-per-evaluation terms (LogisticSoftMax `sum(log, first(beta))` logisticsoftmax.jl:138, the scalar-iteration terms of
 * the Laplace GIGEntropy in AGP_ELBO_REFERENCE mode) are then counted by rank 0 only -- and the hyper-gradient, whose replicated
 * Gaussian-KL part enters with weight 1 / world so that the all-reduced gradient counts it once (agp_svgp_hyper_step_multi; the
 * plain agp_svgp_hyper_step is refused on such a handle).  The batch-mode *_multi calls take rank and world from their
 * communicator themselves, so this call is only needed by hosts that drive the phases (step_local / step_stats / ...) by hand;
 * a handle that is re-created must be told again. */
agp_status agp_svgp_set_batch_shard(agp_svgp* h, int32_t rank, int32_t world);

/* state export / import : VarPosterior(mu, Sigma, eta1, eta2)  src/gpblocks/posterior.jl:21-27 ; any pointer
 * may be NULL.  set_state installs (eta1, eta2) and re-derives (mu, Sigma) (inference.jl:25-28). */
agp_status agp_svgp_get_state(agp_svgp* h, int32_t latent, void* mu, void* sigma, void* eta1, void* eta2);
agp_status agp_svgp_set_state(agp_svgp* h, int32_t latent, const void* eta1, const void* eta2);
/* `cap`: capacity of `out` in rows (AGP_MAT_*) or elements (AGP_VEC_*).  The B-sized outputs refer to the batch of the LAST
 * step / ELBO evaluation (agp_svgp_last_batch) and are refused (AGP_ERR_INVALID) when cap is smaller than that batch;
 * AGP_VEC_ALPHA is state that outlives a batch: min(cap, max_batch) elements are copied. */
agp_status agp_svgp_get_matrix(agp_svgp* h, int32_t latent, int32_t which, void* out, int64_t ldo, int64_t cap);
/* number of points of the last step_local / cavi_step / elbo batch (0 before the first) */
agp_status agp_svgp_last_batch(agp_svgp* h, int64_t* B_host);
/* Data contract of the AnalyticVI (full-batch) kappa cache: Knm / kappa of the last step are reused when the next step is
 * called with the same (x, ldx, idx, B) POINTERS, so X[idx] must not change in place while cached.  A host that refills a
 * buffer (streaming batches through one allocation, mutating a tensor) calls this first.  Stochastic handles never cache. */
agp_status agp_svgp_invalidate_data(agp_svgp* h);
/* init_state(model)  src/training/states.jl:1-9 -- what train! does when it is called WITHOUT a state (training.jl:41-45):
 * local variables as new (LogisticSoftMax alpha = K), RobbinsMonro counters back to 1, new hyper-optimiser (ADAM) states, data
 * caches dropped.  The posterior (eta1, eta2), kernels and Z belong to the model and are kept.  A host that resumes with the
 * state of a previous train! simply does not call it. */
agp_status agp_svgp_init_state(agp_svgp* h);

/* _predict_f (sparse)  src/training/predictions.jl:25-50 : streams over n_t test points without materialising
 * K_*m.  mu_out / var_out : T[n_latent][n_t] (var_out NULL -> cov=false).  n_t = 0 is a successful no-op in every predict_* /
 * proba_y entry point (the reference returns empty arrays). */
agp_status agp_svgp_predict_f(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* mu_out, void* var_out);
/* predict_f(model, X_test; cov=true, diag=false)  predictions.jl:45-49 : full posterior covariance
 *   cov = K** + jitt I - K*m (K^-1 - K^-1 Sigma K^-1) Km*   per latent, cov_out : T[n_latent][n_t][n_t] row-major (mu_out as
 * predict_f).  A multi-output handle returns the MIXED outputs (predictions.jl:52-92): mu_out T[n_task][n_t] = sum_q A[t][q] mu_q,
 * cov_out T[n_task][n_t][n_t] = sum_q A[t][q]^2 cov_q.  K*m IS materialised here (n_t x m), so n_t <= 8192 (AGP_ERR_INVALID
 * beyond). */
agp_status agp_svgp_predict_f_cov(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* mu_out, void* cov_out);

/* ---- PREDICTIVE GRADIENTS (how the prediction changes with the input, over any number of test points) ---------------------------
 * d mu(x*) / d x* and d sigma^2(x*) / d x* of exactly the moments agp_svgp_predict_f returns (no counterpart in the reference):
 * what gradient ascent on an acquisition function, sensitivity analysis and mode finding need, without 2 D finite-difference
 * predictions per point and without the digits those lose on a variance that already cancels.  Per latent, with s the per-dimension
 * scales (ScaleTransform: s_d = s; ARDTransform: s_d = v_d), q_j = sum_d s_d^2 (x_d - z_jd)^2, r_j = sqrt(q_j), v the kernel variance,
 * a = K^-1 mu and A = K^-1 - K^-1 Sigma K^-1 the two objects predict_f uses (exact GP: a = alpha, A = Sigma_y^-1), k* = k(x, Z):
 *   c_j           = v phi'(q_j)                              the derivative of the base function in q = r^2
 *   d mu  / d x_d =  2 s_d^2 sum_j a_j        c_j (x_d - z_jd)
 *   d var / d x_d = -4 s_d^2 sum_j (A k*')_j  c_j (x_d - z_jd)      (k** + jitter is constant in x)
 *   SqExponential phi'(q) = -1/2 e^(-q/2);  Matern32 phi'(q) = -(3/2) e^(-sqrt(3) r);  Matern52 phi'(q) = -(5/6)(1 + sqrt(5) r) e^(-sqrt(5) r)
 * All three are finite at r = 0 and nothing divides by r: a test point that coincides with an inducing point is an ordinary input
 * and that j contributes exactly 0.  The prediction has no prior-mean term in x (predict_f adds none), so neither has the gradient.
 *
 * Outputs: dmu_out, dvar_out (nullable: means only) device T[n_latent][n_t][ldg], ldg >= D in elements; the "Layout" section above
 * holds (ldx >= D, padding never read or written).  A multi-output handle returns the MIXED outputs, as predict_f does:
 * T[n_task][n_t][ldg], d mu_t = sum_q A[t][q] d mu_q, d var_t = sum_q A[t][q]^2 d var_q.
 *
 * How.  Streamed in chunks of 4096 points: K*m (the predictor's kernel-matrix launch) and W = K*m A (one GEMM) when the variances are
 * asked for -- a means-only call forms neither --, then ONE kernel that recomputes q from x and Z by direct differences in ascending
 * d, evaluates c, and contracts a_j c_ij resp. W_ij c_ij against the differences over inducing-point tiles staged through LDS.
 * Double accumulation for both dtypes.  The order of every sum is fixed by (m, D) alone and there are no floating-point atomics: two
 * calls on the same inputs return the same bits.  The workspace is chunk-sized and kept on the handle; nothing grows with n_t.
 *
 * No side effects.  The call completes a pending natural-gradient step first, as every entry point does; after that it uses the
 * predictor's workspace and caches, like agp_svgp_predict_f, and buffers of its own -- the posterior, local variables,
 * agp_svgp_elbo_terms and the status word stay bitwise unchanged.  Asynchronous on the context's stream.
 *
 * Accepted: every single-GPU handle whose agp_svgp_predict_f works -- sparse AnalyticVI / AnalyticSVI (AGP_F64 and AGP_F32), online,
 * AGP_FLAG_FULL, AGP_FLAG_EXACT, AGP_FLAG_NUMERICAL with or without AGP_FLAG_MC, multi-latent (LogisticSoftMax, Heteroscedastic) and
 * multi-output handles.  Refused with AGP_ERR_UNSUPPORTED, by name in agp_last_error, before anything is launched and with the
 * outputs untouched (the handle goes on predicting): AGP_FLAG_SAMPLED; latent-sharded and batch-sharded handles; the
 * ExponentialKernel (not differentiable at zero distance); D > 64 -- the limit of agp_svgp_hypergrad above, for the same reason: the
 * kernel keeps a point's D coordinates and 2 D accumulators in registers across the four waves of a workgroup and stages D-wide
 * tiles in LDS, sized for HB_MAXD.  n_t = 0 is a successful no-op (pointers are then not looked at).  n_t < 0, ldx < D, ldg < D, or
 * (n_t > 0) a NULL xt or dmu_out: AGP_ERR_INVALID, outputs untouched. */
agp_status agp_svgp_predict_f_grad(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* dmu_out,
                                   void* dvar_out /* nullable */, int64_t ldg);

/* ---- ACQUISITION FUNCTIONS (UCB, EI, PI, log EI, log PI of the predictive moments, and their multi-start maximiser on the device) ---
 * The other half of Bayesian optimisation next to "PATHWISE SAMPLING": no counterpart in the reference.  AGP_F64 only.  For one latent
 * let mu(x), var(x) be exactly what agp_svgp_predict_f returns (k** + jitter included) and grad mu, grad var what
 * agp_svgp_predict_f_grad returns.  s = +1, or -1 with `minimize` (the OBJECTIVE is then to be minimised; alpha itself is always
 * maximised), sigma = sqrt(var), z = (s (mu - best) - xi) / sigma, Phi(z) = erfc(-z / sqrt 2) / 2 (never 1 + erf: the left tail is where
 * EI lives), phi(z) = exp(-z^2 / 2) / sqrt(2 pi):
 *   kind                          alpha                       d alpha / d mu      d alpha / d sigma
 *   AGP_ACQ_UCB (beta >= 0)       s mu + beta sigma           s                   beta
 *   AGP_ACQ_EI  (best, xi >= 0)   sigma (z Phi(z) + phi(z))   s Phi(z)            phi(z)
 *   AGP_ACQ_PI  (best, xi >= 0)   Phi(z)                      s phi(z) / sigma    -z phi(z) / sigma
 *   AGP_ACQ_LOG_EI  (best, xi >= 0)   log sigma + log h(z)    s Phi(z) / (sigma h(z))     phi(z) / (sigma h(z))       h(z) = phi(z) + z Phi(z)
 *   AGP_ACQ_LOG_PI  (best, xi >= 0)   log Phi(z)              s phi(z) / (sigma Phi(z))   -z phi(z) / (sigma Phi(z))
 *   grad alpha = d alpha / d mu  grad mu  +  d alpha / d sigma  grad var / (2 sigma)
 * AGP_ACQ_EI and AGP_ACQ_PI are evaluated by their formulas, not in logarithms: they underflow to 0, with a zero gradient, for z below
 * about -38, and an ascent that starts on that plateau does not move.  AGP_ACQ_LOG_EI = AGP_ACQ_LOG | AGP_ACQ_EI and AGP_ACQ_LOG_PI =
 * AGP_ACQ_LOG | AGP_ACQ_PI are their logarithms: the same maximisers, finite with a useful gradient as far as z^2 / 2 is a double, and
 * accepted wherever a kind is (alpha_out, a_out, best_a and ab_out then hold log alpha).  They are accurate to a few units of the
 * last place over the whole range of z: for z > -3 by the expressions of the table (log Phi(z) = log1p(-Phi(-z)) for z > 0), for
 * z <= -3 through Laplace's continued fraction of the Mills ratio with t = -z, cut after the partial numerator 60 (t < 5), 32 (t < 12)
 * or 12 (beyond), where the cut stays below a quarter of a unit of c's last place,
 *   c = 1 / (t + 2 / (t + 3 / (t + ...))),  R = Phi / phi = 1 / (t + c),  h / phi = c R,  log phi = -z^2 / 2 - log sqrt(2 pi)
 * so that log h = log phi + log c + log R, log Phi = log phi + log R, Phi / h = 1 / c, phi / h = 1 / (c R), phi / Phi = t + c, without a
 * cancellation.  alpha = -inf with finite moments and var > 0 only where the exact value lies below -DBL_MAX.  The flag alone
 * (4, which is also AGP_ACQ_LOG | AGP_ACQ_UCB), 3 and 7 stay unknown kinds.
 * var <= 0 takes the limit, it is not left to 0 / 0; with imp = s (mu - best) - xi: UCB alpha = s mu; EI alpha = max(imp, 0) with
 * d alpha / d mu = s where imp > 0 and 0 otherwise; PI alpha = 1 where imp > 0, else 0, with d alpha / d mu = 0; LOG_EI alpha = log imp
 * with d alpha / d mu = s / imp where imp > 0, otherwise alpha = -inf with d alpha / d mu = 0; LOG_PI alpha = 0 where imp > 0, else
 * -inf, with d alpha / d mu = 0; in all five the var term of the gradient is 0.  A NaN moment gives a NaN alpha (and NaN derivatives).
 * -inf is an ordinary value for the best-start rule below (it loses to every finite value); a NaN still never wins.
 *
 * agp_acq_moments  the point function alone on n given moments, device double[n] each: alpha_out, dalpha_dmu (nullable) and
 *   dalpha_dvar (nullable) = d alpha / d sigma / (2 sigma).  n = 0 is a successful no-op.  AGP_ERR_INVALID with a message: ctx or desc
 *   NULL, an unknown kind, beta < 0 or xi < 0, a non-finite beta / best / xi, n < 0, (n > 0) mu, var or alpha_out NULL.
 * agp_svgp_acquisition  alpha_out[i] = alpha(x_i) of latent `latent` and (grad_out nullable) grad_out[i][d] at grad_out + i * ldg + d,
 *   ldg >= D, ldx >= D; the "Layout" section holds (padding never read or written).  Streamed over any n_t in the predictor's chunks
 *   of 4096; per chunk K*m (the predictor's kernel-matrix launch), W = K*m A' (the predictor's GEMM, W_ij = sum_l k*_il A[j][l]), then
 *   ONE kernel that forms q by direct differences in ascending d, evaluates BOTH the base function and its derivative from that q and
 *   accumulates sum_j a_j k_ij (mu), sum_j W_ij k_ij (k*' A k*), and the two contractions of agp_svgp_predict_f_grad over
 *   inducing-point tiles staged through LDS, and a finishing kernel: var = (v + jitter) - k*' A k*, the table, the chain rule.  No
 *   atomics, the order of every sum is fixed by (m, D): the same bits on a repeat, and wherever a point stands in a chunk of the same
 *   length (gemm_nt may pick another kernel for a shorter last chunk: a point's W row may then move by rounding).  No side
 *   effects: the contract is that of agp_svgp_predict_f_grad, paragraph "No side effects".  n_t = 0 is a successful no-op.
 * agp_svgp_acq_maximize  multi-start ADAM ascent of alpha inside the box [lo, hi]: start r < n_starts begins at x0[r] (x0 + r * ldx0,
 *   ldx0 >= D) clipped into the box and takes T = opts->steps steps with g = grad alpha(x).  The recurrences for m, v, mh, vh and x,
 *   the running products b1 / b2, the clipping, "the FINAL iterate, evaluated once more", steps = 0 and the best-start rule (the
 *   largest alpha, ties to the smallest index, a NaN never wins and start 0 does if every value is NaN) are word for word those of
 *   agp_pathwise_maximize ("PATHWISE SAMPLING"), with one sample.  It takes the same agp_pw_ascent_opts; opts->minimize and
 *   opts->x0_shared must be 0 (AGP_ERR_INVALID otherwise): the direction is agp_acq_desc.minimize.  lo, hi and lr are HOST arrays,
 *   validated without a synchronisation and handed to the kernels by value.  Outputs, each nullable (not all): x_out[r][d] at x_out +
 *   r * ldxo + d, a_out[r], best_x[d] (D values), best_a (one double), best_idx (one int64).  One step of a chunk of at most 4096
 *   starts is four launches (K*m, W, the contraction, the ADAM update) on the handle's stream; starts beyond 4096 run chunk after
 *   chunk, each through all T steps.  Asynchronous: no host synchronisation between steps.  The particle state (the iterates and
 *   alpha of every start, the moments of one chunk) belongs to the handle; a call with more starts than any before re-allocates it
 *   (the only place that may wait for the device).  Same bits on a repeat; a start has the same bits wherever it stands among up to
 *   4096 starts (beyond, see the chunks of agp_svgp_acquisition).
 *
 * Both agp_svgp_* calls refuse with AGP_ERR_UNSUPPORTED, by name in agp_last_error, before any launch and with the outputs untouched:
 * AGP_F32 handles; multi-output handles; AGP_FLAG_SAMPLED; latent-sharded and batch-sharded handles; D > 64; a latent with the
 * ExponentialKernel ("ExponentialKernel is not differentiable at zero distance").  AGP_ERR_INVALID with a message: desc, opts or x0
 * NULL; an unknown kind; beta < 0 or xi < 0; a non-finite beta / best / xi; latent outside [0, n_latent); n_t < 0, ldx < D, ldg < D
 * with grad_out given, (n_t > 0) xt or alpha_out NULL; all five outputs NULL; n_starts < 1 or >= 2^31; ldx0 < D; ldxo < D with x_out
 * given; steps outside [0, 65536]; beta1 or beta2 outside [0, 1); eps not finite and positive; lo_host, hi_host or lr_host NULL, a
 * non-finite bound, lo > hi, a step size that is not finite and positive.
 *
 * Pending points (batch acquisition by hallucinated observations: GP-BUCB, Desautels et al. 2014, "kriging believer").  The posterior
 * is conditioned on the pending points at their own predicted mean: the mean stays, the variance shrinks, and q points are picked
 * greedily, each conditioned on those before.  This is for one latent with kernel k, kernel variance v, inducing / training inputs Z
 * (m points) and the predictor (a, A) of AGP_VEC_APRED / AGP_MAT_APRED.  mu(x) = k*(x)' a and var(x) = v + jitter - k*(x)' A k*(x)
 * are exactly what agp_svgp_predict_f returns.  The posterior covariance of the latent is cov(x, x') = k(x, x') - k*(x)' A k*(x').
 * It carries no jitter.  Take pending points P = (p_1 ... p_n) and a fantasy-noise variance tau2 >= 0 (`noise`):
 *   C_ij   = cov(p_i, p_j) + (jitter + tau2) [i == j]          n x n
 *   c_j(x) = cov(x, p_j)
 *   mu_P(x)  = mu(x)
 *   var_P(x) = var(x) - c(x)' C^-1 c(x)
 *   alpha_P(x) = A(mu(x), var_P(x))           the table above, unchanged
 *   grad alpha_P by the chain rule, with grad var_P = grad var - 2 (dc/dx)' C^-1 c
 * This is the posterior after observing mu(P) at P with noise tau2.  For an exact GP with noise sigma^2 and tau2 = sigma^2, it equals
 * the GP refitted on (X u P, y u mu(P)) with fixed hyper-parameters.  Equivalent form, the one that is computed: augment the predictor,
 *   Z'  = [Z; P]
 *   a'  = [a; 0]
 *   A'  = [[A + V C^-1 V', -V C^-1], [-C^-1 V', C^-1]],   V = A K_ZP
 *   var_P(x) = (v + jitter) - k'(x)' A' k'(x)
 * and the per-step kernels of agp_svgp_acquisition / agp_svgp_acq_maximize run unchanged on (Z', a', A') with m' = m + n.
 * Bordering order: A' is always built by bordering, one point at a time in the order p_1, p_2, ....  Given the current (Z', A') of
 * size n' and a new point p:
 *   k' = k(Z', p)
 *   w  = A' k'
 *   c  = (v + jitter + tau2) - k'' w            (k'' is the transpose of k')
 *   A'' = [[A' + w w'/c, -w/c], [-w'/c, 1/c]]
 * The update is kept in its factors, not summed into one matrix: with u = [w; -1], A'' = A' + u u'/c, and stored are A0 = [[A, 0], [0, 0]],
 * the u_b and the -u_b / c_b, so that A' k' = A0 k' + sum_b u_b (u_b' k') / c_b and, per pass, W = K*m' A0^T + (K*m' U^T) (U / c)^T (three
 * GEMMs where the calls above have one).  The entries of a summed A' reach 1 / c and k'' A' k' would lose eps |A'| |k'|^2 absolutely --
 * 1e-9 of the variance with 63 pending points around one inducing point, which EI and PI magnify --; in the factors an error of u_b' k'
 * enters var_P multiplied by u_b' k' itself, which is small where c_b is.
 * A pending set passed in by the caller and a set accumulated during a batch therefore give the same bits.  c <= 0 or a non-finite c
 * cannot happen with jitter > 0 in exact arithmetic; it is handled like a non-SPD factorisation: latched on the handle and reported
 * by agp_svgp_check_status (AGP_ERR_NOT_POSDEF).  Every sum of the bordering has an order fixed by n'; no atomics, nothing waits.
 * The augmented predictor lives in workspaces of its own, sized once for m + AGP_ACQ_MAX_PENDING points: nothing that
 * agp_svgp_predict_f, agp_svgp_predict_f_grad, agp_svgp_acquisition or agp_svgp_acq_maximize use is resized or overwritten.
 *
 * agp_svgp_acquisition_pending  agp_svgp_acquisition with alpha_P and grad alpha_P: xp holds the n_pending points (device, row i at
 *   xp + i * ldp, ldp >= D), noise = tau2.  With n_pending = 0 it is agp_svgp_acquisition, launch for launch and bit for bit (xp is
 *   then not looked at).
 * agp_svgp_acq_maximize_batch  q rounds.  Round b = 0 ... q - 1 runs the ascent of agp_svgp_acq_maximize -- the same recurrence, the
 *   same x0, the same best-start rule and the same chunks of 4096 -- on alpha_P with P = pending u {x_0 ... x_{b-1}}.  xb_out[b] (at
 *   xb_out + b * ldxb, ldxb >= D) is the round's best final iterate, ab_out[b] (nullable) alpha_P there, idxb_out[b] (nullable, int64)
 *   the index of the winning start.  The whole call is enqueued on the handle's stream with no host synchronisation between steps or
 *   between rounds: the host knows every size in advance, and the winner moves device to device into the pending list.  The only
 *   wait is a first-time or growing allocation, as in agp_svgp_acq_maximize.  With n_pending = 0 and q = 1 the outputs have the bits
 *   of best_x / best_a / best_idx of agp_svgp_acq_maximize; a batch of q equals q chained calls with q = 1, each given the earlier
 *   winners as extra pending points; a repeat of any call gives the same bits.  No side effects, as above.
 * Both refuse (AGP_ERR_UNSUPPORTED) the same handles in the same words as the two calls above, before any launch and with the outputs
 * untouched.  AGP_ERR_INVALID with a message: everything the two calls above check; n_pending < 0, q < 1 or n_pending + q >
 * AGP_ACQ_MAX_PENDING; noise negative or not finite; xp NULL with n_pending > 0; ldp < D (n_pending > 0); ldxb < D; xb_out NULL.
 * Pending coordinates are device data and are not validated (the kernel functions clamp a squared distance that is not a positive
 * number to 0, so a NaN coordinate does not reliably show as a NaN value).
 *
 * Joint batches (Monte-Carlo q-EI and q-UCB with a joint reparameterised sample; Wilson et al. 2018, BoTorch's qExpectedImprovement
 * and qUpperConfidenceBound).  The greedy batch above picks point b without knowing where the later ones go; the joint criterion is a
 * function of all q points together, under their posterior correlation.  This is for one latent with the predictor (a, A) and a set
 * of q' = q + n points x_1 ... x_q, p_1 ... p_n: the q points are optimised, the n points are pending and fixed.  Pending points here
 * are members of the joint sample, as BoTorch's X_pending: they are NOT hallucinated observations, so a fantasy noise has no meaning
 * and does not appear.  With k*(x) = k(Z, x), base samples eps (S x q', the caller's) and s = -1 with `minimize`:
 *   mu_j  = k*(x_j)' a
 *   C_jl  = k(x_j, x_l) - k*(x_j)' A k*(x_l) + jitter [j == l]          q' x q'
 *   C     = L L'   (lower Cholesky)
 *   f_s   = mu + L eps_s
 *   q-EI   (AGP_ACQ_EI)    alpha = (1/S) sum_s max(0, max_j (s (f_sj - best) - xi))
 *   q-UCB  (AGP_ACQ_UCB)   alpha = (1/S) sum_s max_j (s mu_j + beta sqrt(pi/2) |(L eps_s)_j|)
 * The diagonal of C is exactly the variance of agp_svgp_predict_f and C is the matrix agp_svgp_predict_f_cov returns at those points.
 * With q' = 1 the expectation of q-UCB over eps is s mu + beta sigma, and that of q-EI is EI.  The first maximum wins a tie.  The
 * gradient is the sub-gradient through the winning member.  A sample counts for q-EI if its maximum is positive, always for q-UCB:
 *   mu-bar_j  = (s/S) #{s : j wins and the sample counts}
 *   L-bar_jk  = (1/S) sum over those samples of g_s eps_sk,  k <= j;   g_s = s (q-EI),  g_s = sign((L eps_s)_j) beta sqrt(pi/2) (q-UCB)
 *   Phi       = tril(L' L-bar) with the diagonal halved,   C-bar = sym(L^-T Phi L^-1)          (the Cholesky backward)
 *   V_j       = mu-bar_j a - 2 sum_l C-bar_jl W_l          over all q' members l;  W_l = A k*(x_l), the row of W = K*m A' of x_l or p_l
 *   d alpha / d x_j = sum_i V_ji d k(x_j, z_i) / d x_j + 2 sum_l C-bar_jl d1 k(x_j, x_l)
 * Pending members get no gradient and do not move.  The criterion has kinks where a sample's winner changes or its improvement
 * changes sign; there the sub-gradient of the first maximum is returned.  eps is a device pointer, double [S][lde] with lde >= q + n,
 * row s holding the draws of x_1 ... x_q, p_1 ... p_n in that order.  The same table serves every start and every step
 * (sample-average approximation): the library draws nothing and its random streams are untouched (agp_mc_normals fills such a table).
 *
 * agp_svgp_acquisition_joint  alpha_out[r] of n_sets sets, member j of set r at xq + (r q + j) ldx, and (grad_out nullable) its
 *   gradient in the same layout with ldg.  Sets are streamed in chunks of floor(4096 / q): a tuple never straddles two chunks.  Per
 *   chunk: K*m and W of the chunk's points (the two launches of agp_svgp_acquisition), the covariance kernel (mu and C of a set from
 *   its rows of K*m and W), the per-set kernel (Cholesky, samples, alpha, the backward pass to mu-bar and C-bar), the weight rows V
 *   with the point-to-point term, the contraction of agp_svgp_acquisition on V, and a finishing kernel: seven launches, four without
 *   the gradient.  K*m and W of the pending points are formed once per call.  n_sets = 0 is a successful no-op.
 * agp_svgp_acq_maximize_joint  the ascent of agp_svgp_acq_maximize on alpha: the same ADAM recurrence per coordinate, the same
 *   clipping, "the FINAL iterate of the best start", the same agp_pw_ascent_opts and checks.  A start is a q-tuple: member j of start
 *   r at x0 + (r q + j) ldx0.  Outputs, each nullable (not all): x_out in that layout with ldxo, a_out[r], best_x (q rows, row j at
 *   best_x + j ldb), best_a, best_idx.  No host synchronisation between steps.
 * A Cholesky pivot that is not positive and finite cannot happen with jitter > 0 in exact arithmetic; it is latched on the handle and
 * reported by agp_svgp_check_status (AGP_ERR_NOT_POSDEF), as the bordering does it.  Every sum has an order fixed by (m, D, q', S);
 * no atomics: the same bits on a repeat, and a start has the same bits wherever it stands in a chunk of the same length.  Nothing that
 * agp_svgp_predict_f, agp_svgp_predict_f_grad, agp_svgp_acquisition* or agp_svgp_acq_maximize* use is resized or overwritten.
 * Both refuse (AGP_ERR_UNSUPPORTED) the same handles in the same words as agp_svgp_acq_maximize, and by name AGP_ACQ_PI,
 * AGP_ACQ_LOG_EI and AGP_ACQ_LOG_PI (the joint PI has a zero gradient almost everywhere, the log kinds need a smoothed maximum),
 * before any launch and with the outputs untouched.  AGP_ERR_INVALID with a message: everything agp_svgp_acquisition and
 * agp_svgp_acq_maximize check; q < 1; n_pending < 0; q + n_pending > AGP_ACQ_JOINT_MAX_Q; S outside [1, 4096]; eps NULL; lde < q +
 * n_pending; xp NULL or ldp < D with n_pending > 0; a leading dimension < D; a NULL required output.
 *
 * Out of scope: the joint PI and the joint log kinds, fantasies that move the mean, Float32, multi-output and sharded
 * handles, a single-launch ascent. */
#define AGP_ACQ_MAX_PENDING 64 /* n_pending + q; an interface limit, not a tuned value */
#define AGP_ACQ_JOINT_MAX_Q 16 /* q + n_pending of a joint batch; an interface limit, not a tuned value */
enum { AGP_ACQ_UCB = 0, AGP_ACQ_EI = 1, AGP_ACQ_PI = 2, AGP_ACQ_LOG = 4 /* a flag on EI and PI: */, AGP_ACQ_LOG_EI = 5, AGP_ACQ_LOG_PI = 6 };
typedef struct {
  int32_t kind;     /* AGP_ACQ_* */
  int32_t minimize; /* 0: the objective is maximised, 1: minimised (s = -1) */
  double beta;      /* UCB */
  double best, xi;  /* EI, PI: the incumbent and the margin */
} agp_acq_desc;
agp_status agp_acq_moments(agp_ctx* ctx, const agp_acq_desc* desc, int64_t n, const void* mu, const void* var, void* alpha_out,
                           void* dalpha_dmu /* nullable */, void* dalpha_dvar /* nullable */);
agp_status agp_svgp_acquisition(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xt, int64_t ldx, int64_t n_t,
                                void* alpha_out, void* grad_out /* nullable */, int64_t ldg);
/* (agp_svgp_acq_maximize is declared under "PATHWISE SAMPLING", below the agp_pw_ascent_opts it takes) */
/* predict_y  predictions.jl:178-198 : regression (Gaussian, StudentT, Laplace, Heteroscedastic) -> T[n_t] mean ;
 * logistic / BayesianSVM -> int32[n_t] (mu_f > 0) ; Poisson / NegBinomial -> T[n_t] expected count (predictions.jl:211) ;
 * LogisticSoftMax -> int32[n_t] argmax_k mu_f,k (0-based LOCAL latent index + latent_offset) */
agp_status agp_svgp_predict_y(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* y_out);
/* ---- OnlineSVGP (src/models/OnlineSVGP.jl, src/training/onlinetraining.jl) ------------------------------------------------
 * A streaming model is a sequence of handles: when a batch arrives the caller snapshots the current posterior, picks the
 * new inducing points (InducingPoints.OIPS on its side, with agp_kernelmatrix for the kernel values), creates a handle
 * for the new Z and installs the previous posterior as its prior.  Only AnalyticVI() (stochastic = 0) is accepted: the
 * reference's stochastic branch is dead code (onlinetraining.jl:52 uses an undefined name).
 *
 * agp_svgp_online_snapshot: save_old_gp! (onlinetraining.jl:170-180): invDa_out (m x m, ld ldi) = -2 eta2 - inv(K),
 *   eta1_out (m) = eta1, *prevLa_host = (-logdet Sigma + logdet K - mu'eta1)/2.  Device outputs; synchronises.
 * agp_svgp_set_online_prior: previous_gp of the opt state + Z_a of the latent.  za = NULL: first batch (Z_a empty:
 *   kappa_a = I, K_ab = 0, K~_a = 0; pass invDa = I, prev_eta1 = 0, prevLa = 0 as init_opt_state does, states.jl:85-97;
 *   ma must equal m).  From then on every step uses the online natural gradient (analyticVI.jl:183-203)
 *     eta1 = K\mu0 + kappa' grad_E_mu + kappa_a' eta1_a ;  eta2 = -(kappa' diag(grad_E_Sigma) kappa + kappa_a' invD_a kappa_a/2 + inv(K)/2)
 *   and agp_svgp_elbo subtracts extraKL (KLdivergences.jl:30-54).
 * agp_svgp_adopt_local: dst takes src's local variables and expectation gradients (same likelihood / max_batch / ctx):
 *   the first iteration on a new batch updates the local variables under the OLD inducing points (compute_old_matrices,
 *   onlinetraining.jl:78-104): run agp_svgp_step_local on the old handle, then on the new one
 *   agp_svgp_step_local + agp_svgp_adopt_local(new, old) + agp_svgp_step_stats(fused) + agp_svgp_step_global. */
agp_status agp_svgp_online_snapshot(agp_svgp* h, int32_t latent, void* invDa_out, int64_t ldi, void* eta1_out,
                                    double* prevLa_host);
agp_status agp_svgp_set_online_prior(agp_svgp* h, int32_t latent, const void* za, int64_t ldza, int64_t ma, const void* invDa,
                                     int64_t ldi, const void* prev_eta1, double prevLa);
agp_status agp_svgp_adopt_local(agp_svgp* dst, agp_svgp* src);
/* the whole first iteration on a new batch (onlinetraining.jl:78-104) in one call: h_old.step_local(x, y) [+ the
 * LogisticSoftMax fixed point] ; h_new.step_local ; adopt_local(h_new, h_old) ; h_new natural gradient + global update */
agp_status agp_svgp_online_first_step(agp_svgp* h_new, agp_svgp* h_old, const void* x, int64_t ldx, const void* y,
                                      int64_t B);
/* Gauss-Hermite rule used INSIDE training by PoissonLikelihood's lambda update (expectation(logistic, mu, sigma2),
 * src/functions/utils.jl:16-19 ; same nodes as predictions.jl:4: x*sqrt2, w/sqrt(pi)).  Must be called before the first
 * step of a Poisson handle; other likelihoods ignore it. */
agp_status agp_svgp_set_quadrature(agp_svgp* h, const double* gh_nodes_host, const double* gh_weights_host,
                                   int32_t n_nodes);
/* likelihood state: the lambda of Poisson (poisson.jl:78) / Heteroscedastic (heteroscedastic.jl:95), which every local
 * update re-estimates; other likelihoods: get returns p0, set is AGP_ERR_INVALID.  get synchronises. */
agp_status agp_svgp_get_lik_param(agp_svgp* h, double* value_host);
/* LogisticSoftMax: the Gamma shape alpha of the local variables is the one piece of local state the reference carries from
 * one minibatch to the next (logisticsoftmax.jl:65-72 starts its fixed point from the previous alpha); read it with
 * agp_svgp_get_matrix(AGP_VEC_ALPHA), restore it here (device pointer, n <= max_batch) when resuming a saved model. */
agp_status agp_svgp_set_lsm_alpha(agp_svgp* h, const void* alpha, int64_t n);
agp_status agp_svgp_set_lik_param(agp_svgp* h, double value);
/* proba_y  predictions.jl:225-247 + compute_proba : Gaussian / StudentT / Laplace / Heteroscedastic -> (mean, var) ;
 * BayesianSVM / Poisson / NegBinomial -> (E[link(f)], Var) by Gauss-Hermite like logistic ; logistic -> (p, var) by
 * Gauss-Hermite with the caller's nodes/weights (predictions.jl:4 : x*sqrt2, w/sqrt(pi), 100 nodes) ;
 * LogisticSoftMax -> out0 = T[n_t][K] normalised logistic(mu_f) (multiclass.jl:96-117), out1 unused. */
agp_status agp_svgp_proba_y(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, const double* gh_nodes_host,
                            const double* gh_weights_host, int32_t n_nodes, void* out0, void* out1);

/* ---- Gibbs sampling (AGP_FLAG_FULL | AGP_FLAG_SAMPLED) ----------------------------------------------------------------------
 * One sweep at counter t, for the single latent (sampling.jl:36-75, gibbssampling.jl:44-60):
 *     theta_i ~ p(omega_i | f_i, y_i)                      sample_local!   logistic.jl:53-60: PG(1, |f_i|) ; negativebinomial.jl:83-90:
 *                                                          PG(y_i + r, |f_i|) ; studentt.jl:84-92: omega_i ~ InverseGamma((nu + 1) / 2,
 *                                                          ((f_i - y_i)^2 + sigma^2 nu) / 2), theta_i = 1 / omega_i
 *     Sigma = inv(2 Diagonal(grad_E_Sigma) + inv(K))       sample_global!  with grad_E_mu, grad_E_Sigma = theta / 2 of the likelihood
 *     f ~ N(Sigma (grad_E_mu + K \ mu0), Sigma)            as f = Xa' (Xa eta1 + z), Xa = chol(Sigma^-1)^-1 (lower), z ~ N(0, I)
 *
 * RANDOM STREAMS -- the contract that lets a host program reproduce a chain (tests/_mcgp_ref.py does).
 *   Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, ten rounds).
 *   Key (k0, k1) = (seed & 0xffffffff, seed >> 32).  Counter (c0, c1, c2, c3) = (i, t, stream, j): i the 0-based point index, t the
 *   sweep counter, stream 0 = the local variables of point i, stream 1 = the normal draw z_i, j = 0, 1, 2, ... the block number.
 *   Block j yields the words (w0, w1, w2, w3) and from them two uniforms, u_2j from (w0, w1) and u_2j+1 from (w2, w3):
 *       k = (hi >> 5) << 26 | (lo >> 6)   (53 bits),   u = (k + 0.5) 2^-53,   so 0 < u < 1.
 *   A stream is consumed strictly in the order u_0, u_1, u_2, ...  Derived variates:
 *       Exponential  E = -log(u)                                (one uniform)
 *       Normal       N = sqrt(-2 log a) cos(2 pi b)             (two uniforms a then b; the sine value is NOT used;
 *                                                                2 pi = 6.283185307179586 multiplied onto b in double)
 *   z_i of sweep t = Normal from stream 1 (block 0 only).  All comparisons below are in double, NaN-free.
 *   PG(1, c) -- Devroye's alternating series as sample_pg1 states it (ComplementaryDistributions/polyagamma.jl:139-166), T = 0.64:
 *       z = |c| / 2, K = pi^2 / 8 + z^2 / 2, r = mass_texpon(z) = 1 / (1 + (4 / pi)(exp(x0 - z + logPhi(b)) + exp(x0 + z + logPhi(a)))),
 *       x0 = log K + K T, b = 1.25 (T z - 1), a = -1.25 (T z + 1), logPhi(x) = log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 for x < 0 and
 *       log1p(-erfc(x / sqrt 2) / 2) otherwise.
 *       repeat:  u = U; if r > u: x = T + E / K, else x = TIG(z)
 *                S = a(0, x); y = U S; for n = 1, 2, ...: n odd: S -= a(n, x), accept (return x / 4) unless y > S;
 *                                                         n even: S += a(n, x), reject (repeat) if y > S
 *       a(n, x) = k exp(-k^2 x / 2) for x > T, else exp(-1.5 (log(pi / 2) + log x) + log k - 2 (n + 1/2)^2 / x), k = (n + 1/2) pi.
 *       TIG(z), mu = 1 / z (z = 0: infinity):
 *         mu > T:  repeat { repeat { E = Exp, E' = Exp } while E^2 > 2 E' / T;  x = T / (1 + E T)^2;  u = U } while u > exp(-z^2 x / 2)
 *         else:    repeat { Y = N^2; w = mu Y; x = mu + mu w / 2 - (mu / 2) sqrt(4 w + w^2); u = U; if u > mu / (mu + x): x = mu^2 / x }
 *                  while x > T
 *   PG(b, c), integer b >= 1: r once, then the sum of b draws of PG(1, c) from the same stream, one after the other
 *       (draw_sum, polyagamma.jl:59-61); b = y_i + r of the NegBinomial likelihood, at most 65536.
 *   InverseGamma(alpha, beta) = beta / G, G ~ Gamma(alpha, 1) by Marsaglia & Tsang: a' = alpha + 1 if alpha < 1 else alpha,
 *       d = a' - 1/3, c = 1 / sqrt(9 d);  repeat { z = N; v1 = 1 + c z; if v1 <= 0 continue; v = v1^3; u = U;
 *       accept if u < 1 - 0.0331 z^4, else accept if log u < z^2 / 2 + d (1 - v + log v) };  G = d v;  if alpha < 1: G *= exp(log(U) / alpha).
 *   Every loop has an iteration bound (1000 rounds, 64 series terms) that a correct sampler does not reach; reaching it latches a
 *   failure that agp_svgp_check_status reports as AGP_ERR_HIP.
 *
 * agp_svgp_gibbs_sample runs discard_initial + 1 + (n_samples - 1) * thinning sweeps and keeps sweep
 *   discard_initial + 1 + k * thinning (1-based within the call), k = 0 .. n_samples - 1, writing the kept f into store[k][0 .. N)
 *   (device, leading dimension lds >= N).  This kept-sweep convention is OURS: the reference delegates it to AbstractMCMC.jl, which is
 *   not part of its sources (mcmcsample keeps the first sample after discard_initial and every thinning-th after it).  y: T[N] as for
 *   cavi_step (NegBinomial: integer counts).  The whole chain is enqueued without a host synchronisation between sweeps (the first
 *   call refreshes K, which synchronises once); failures -- a non-SPD matrix, a loop bound -- are latched and reported by
 *   agp_svgp_check_status.  The sweep counter t lives in the handle and continues over calls: with one seed, two calls of S sweeps
 *   give bit for bit the chain of one call of 2 S (the reference's cat = true).  t + sweeps must stay below 2^32.
 * agp_svgp_gibbs_counter reads (set = 0) or sets (set = 1) the sweep counter (save / load).
 * agp_sample_local is sample_local! on caller-supplied f outside any model -- the same kernel: theta_out[i] (and aux_out[i], nullable:
 *   |f_i|, StudentT omega_i) drawn from stream 0 of (seed, t, i).  Float64 device pointers; lik->kind one of the three likelihoods
 *   above; synchronises and reports a loop bound itself.  With AGP_LIK_LOGISTIC it is the reference's exported PolyaGamma(1, c) sampler.
 * agp_svgp_predict_samples is _predict_f(::MCGP) / proba_y(::MCGP) (predictions.jl:94-130, 260-276) on a store of n_samples kept
 *   samples (device, [n_samples][lds]): F* = K*n (K \ F) for all samples (_sample_f), test points in blocks of the handle's
 *   prediction workspace (K*n is never held whole), then per test point, over the samples:
 *     mode 0  out0 = mean f*
 *     mode 1  out0 = mean f*, out1 = k** + jitt - diag(K*n K^-1 Kn*) + var f*      (the intended form of predictions.jl:115)
 *     mode 2  out0, out1 = mean and variance of logistic(f*)                        (AGP_LIK_LOGISTIC only)
 *   var is the sample variance (n - 1; NaN for one sample).  out0 / out1: T[n_t].  At most 65536 samples per call (AGP_ERR_INVALID
 *   with a message beyond: the workspace holds F K^-1 of every sample of a call).
 * NegBinomial targets must be non-negative integers: anything else is latched by the sweep (and reported by agp_sample_local) as
 *   AGP_ERR_LABELS. */
agp_status agp_svgp_gibbs_sample(agp_svgp* h, const void* y, int64_t n_samples, int64_t discard_initial, int64_t thinning,
                                 uint64_t seed, void* store, int64_t lds);
agp_status agp_svgp_gibbs_counter(agp_svgp* h, int32_t set, int64_t* t_host);
agp_status agp_sample_local(agp_ctx* ctx, const agp_lik_desc* lik, const void* y, const void* f, int64_t n, uint64_t seed, int64_t t,
                            void* theta_out, void* aux_out);
agp_status agp_svgp_predict_samples(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, const void* store, int64_t lds,
                                    int64_t n_samples, int32_t mode, void* out0, void* out1);

/* ---- NUMERICAL INFERENCE (AGP_FLAG_NUMERICAL, with AGP_FLAG_FULL or with no other model flag) ---------------------------------------
 * VGP(X, y, kernel, likelihood, QuadratureVI()) (with AGP_FLAG_FULL) and SVGP(kernel, likelihood, QuadratureVI() / QuadratureSVI(B), Z)
 * (without)  src/inference/numericalVI.jl, src/inference/quadratureVI.jl.  Float64, one latent (K latents with AGP_FLAG_MC: "MC INTEGRATION" below),
 * likelihoods AGP_LIK_LOGISTIC, AGP_LIK_STUDENTT, AGP_LIK_LAPLACE; a Gaussian likelihood is refused as "not compatible"
 * (test/likelihood/gaussian.jl:38,59), every other likelihood, AGP_F32, AGP_FLAG_EXACT and AGP_FLAG_SAMPLED with
 * AGP_ERR_UNSUPPORTED.  The formulas below are the full model's (kappa = I, K~ = 0, rho = 1); the sparse model's follow them.  The handle keeps (mu, Sigma) itself (mu = 0, Sigma = I at
 * creation) and the optimiser's moments of both, not (eta1, eta2).  One step, with (x_j, w_j) the rule the host installed:
 *     mu_f = mu ; var_f = diag Sigma                                  latentgp.jl:171-189
 *     f_ij = mu_f,i + sqrt(max(var_f,i, 0)) x_j                       quadratureVI.jl:118
 *     g_i = sum_j w_j l'(y_i, f_ij) ; h_i = sum_j w_j l''(y_i, f_ij)  (grad_E_mu = g, grad_E_Sigma = h / 2)
 *     grad_eta1 = g - K^-1 (mu - mu0) ; grad_eta2 = Diagonal(h / 2) - (K^-1 - Sigma^-1) / 2          numericalVI.jl:121-134
 *     natural:  grad_eta2 <- 2 Sigma grad_eta2 Sigma ; grad_eta1 <- K grad_eta1                      numericalVI.jl:152-156
 *               formed as (Sigma Diagonal(h) - Sigma K^-1) Sigma + Sigma and K g - (mu - mu0): no inverse of Sigma
 *     d mu, d Sigma = rule(grad) ; mu <- mu + d mu                                                  numericalVI.jl:158-166
 *     alpha = 1 ; while Sigma + alpha Symmetric(d Sigma) is not positive definite and alpha > 1e-8: alpha /= 2
 *     alpha > 1e-8 ? Sigma <- Sigma + alpha Symmetric(d Sigma) : Sigma unchanged (mu has moved)      numericalVI.jl:167-175
 *   Symmetric reads the upper triangle.  Positive definite = the library's Cholesky factorisation meets no non-positive pivot; the
 *   status word is read by the host once per attempt, so a step synchronises at least once.  The accepted factor is kept (log det
 *   Sigma of the ELBO; its inverse gives Sigma^-1 of the classical gradient).
 *   rule (opt_kind = AGP_OPT_*): Descent d = eta g ; Momentum vel = p1 vel + eta g, d = vel ; ADAM m = p1 m + (1 - p1) g,
 *   v = p2 v + (1 - p2) g^2, d = eta (m / (1 - p1^t)) / (sqrt(v / (1 - p2^t)) + eps), t = 1, 2, ... the step number.
 *   The likelihood terms, with three definitions of the reference restated in their intended form (no bug-compatible mode):
 *     Logistic (y in {-1, 1})   l = -log(1 + exp(-y f)), l' = y sigma(-y f), l'' = -sigma(f) sigma(-f)
 *                               (logistic.jl:98-100 returns -exp(y f) / logistic(-y f)^2, which grows like exp(3 |f|))
 *     StudentT (nu, sigma)      the density as written (studentt.jl:43-46), u = (y - f) / sigma, a = (nu + 1) / 2:
 *                               l = log Gamma(a) - log sqrt(nu pi) - log Gamma(nu / 2) - a log(1 + u^2),
 *                               l' = 2 a u / (sigma (1 + u^2)), l'' = -2 a (1 - u^2) / (sigma^2 (1 + u^2)^2)
 *     Laplace (beta)            l = -|y - f| / beta - log(2 beta), l' = sign(y - f) / beta by quadrature;
 *                               h_i = -(2 / beta) N(y_i; mu_f,i, var_f,i) in closed form (the second derivative is a delta function;
 *                               laplace.jl:131 returns +1 / sqrt(2 pi var) / beta^2: wrong sign, no exponential); 0 where var_f <= 0
 *     clipping                  not offered: the clipping branch of quadratureVI.jl:121-126 returns values of the opposite sign
 *                               convention to the unclipped one
 * (The entry point that installs the rule is agp_svgp_nvi_configure, not a second form of agp_svgp_set_quadrature: that name is
 *   taken by the Gauss-Hermite rule of the predictions and of the Poisson likelihood, with another signature.)
 * agp_svgp_nvi_configure installs the rule of n nodes x_j = sqrt(2) t_j and weights w_j = omega_j / sqrt(pi) ((t, omega) the
 *   Gauss-Hermite rule; host arrays, copied: the device and a host restatement share them bit for bit), natural != 0 for the natural
 *   gradient, and the optimiser (eta; p1, p2, eps as above, ignored where the rule has none).  It may be called again at any time; the
 *   moments are kept.
 * The sparse model (no AGP_FLAG_FULL; m inducing points, max_batch >= B; desc.stochastic is accepted and not read) sees a minibatch
 *   through K_nm, kappa = K_nm K^-1, K~ = k_ii + jitt - diag(kappa K_mn) and rho = N / B (latentgp.jl:171-212, numericalVI.jl:136-150):
 *     mu_f = kappa mu ; var_f = diag(kappa Sigma kappa') + K~
 *     grad_eta1 = rho kappa' g - K^-1 (mu - mu0) ; grad_eta2 = rho kappa' Diagonal(h / 2) kappa - (K^-1 - Sigma^-1) / 2
 *     natural: formed as K (rho kappa' g) - (mu - mu0) and rho W Diagonal(h) W' - Sigma K^-1 Sigma + Sigma with W = Sigma kappa'
 *   The kernel matrices of the batch are recomputed every step and every ELBO evaluation; there is no look-ahead (agp_svgp_prefetch
 *   is refused like the CAVI phases).  ELBO = rho sum over the batch - GaussianKL.
 * agp_svgp_nvi_step: the full model takes the whole training set -- y T[N], idx = NULL, B = N, rho = 1 (anything else:
 *   AGP_ERR_BAD_BATCH / AGP_ERR_INVALID); x is not read (the inputs are the handle's Z) and may be NULL.  The sparse model takes
 *   (x, ldx, y, idx, B, rho) with the meaning they have for agp_svgp_cavi_step: x T[N][ldx], ldx >= D, y T[N] read at idx (NULL:
 *   the first B points), B <= max_batch, rho > 0.
 * agp_svgp_nvi_info reports alpha of the last step, the halvings and the rejected updates (alpha <= 1e-8) since creation.
 * agp_svgp_nvi_state reads (set = 0) or installs (set = 1) the moments -- mom_mu double[2][N], mom_sigma double[2][N][N], device,
 *   contiguous; slot 0 Momentum's velocity / ADAM's m, slot 1 ADAM's v; only the upper triangle of a mom_sigma slot is live -- and the
 *   step counter t.  With get_state / set_state this is everything a saved model continues from bit for bit.
 * The other entry points on such a handle:
 *   get_state       mu, sigma; eta1 / eta2 must be NULL (AGP_ERR_UNSUPPORTED)
 *   set_state       eta1 = mu T[N], eta2 = Sigma T[N][N] (contiguous); Sigma not positive definite: AGP_ERR_NOT_POSDEF
 *   elbo            rho sum_i sum_j w_j l(y_i, f_ij) - GaussianKL at the current posterior (numericalVI.jl:193-206); fresh_local is
 *                   ignored (there are no local variables); elbo_enqueue evaluates synchronously; elbo_terms = (sum, KL, 0)
 *   predict_f / predict_f_cov / predict_y / proba_y, set_kernel, set_prior_mean, refresh_K, check_status: as for VGP
 *   init_state      new optimiser moments, t = 0; the posterior is kept
 * Refused with AGP_ERR_UNSUPPORTED on top of AGP_FLAG_FULL's list (which a sparse numerical handle shares: the CAVI phases,
 * prefetch, shards, K_nm / kappa of get_matrix): cavi_step, hypergrad, hyper_step, hyper_apply, hyper_configure,
 * hyper_rule (the hyper-parameter step through the quadrature ELBO is not built).
 * agp_quad_expectations is the quadrature kernel on caller-supplied moments outside any model: ell_i = sum_j w_j l(y_i, f_ij), g_i, h_i
 *   for n_pts points (y, mu, var, ell, g, h: double[n_pts], device; nodes, weights: double[n], host); synchronises. */
agp_status agp_svgp_nvi_configure(agp_svgp* h, int32_t n, const double* nodes_host, const double* weights_host, int32_t natural,
                                  int32_t opt_kind, double eta, double p1, double p2, double eps);
agp_status agp_svgp_nvi_step(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho);
agp_status agp_svgp_nvi_info(agp_svgp* h, int32_t latent, double* alpha_last_host, int64_t* halvings_total_host,
                             int64_t* rejected_total_host);
agp_status agp_svgp_nvi_state(agp_svgp* h, int32_t latent, int32_t set, void* mom_mu, void* mom_sigma, int64_t* t_host);
agp_status agp_quad_expectations(agp_ctx* ctx, const agp_lik_desc* lik, const void* y, const void* mu, const void* var, int64_t n_pts,
                                 const double* nodes_host, const double* weights_host, int32_t n, void* ell, void* g, void* h);

/* ---- MC INTEGRATION (AGP_FLAG_NUMERICAL | AGP_FLAG_MC, with or without AGP_FLAG_FULL) ---------------------------------------------------
 * VGP(X, y, kernel, likelihood, MCIntegrationVI()) and SVGP(kernel, likelihood, MCIntegrationVI() / MCIntegrationSVI(B), Z)
 * src/inference/MCVI.jl, for the multi-class likelihoods AGP_LIK_SOFTMAX (src/likelihood/softmax.jl) and AGP_LIK_LOGISTICSOFTMAX
 * (src/likelihood/logisticsoftmax.jl:144-193): Float64, n_latent = n_class = K with 2 <= K <= 64 (one wave holds the K latents of a
 * draw).  AGP_FLAG_MC without AGP_FLAG_NUMERICAL, any other likelihood, K = 1 and AGP_F32 are AGP_ERR_UNSUPPORTED with a message.
 * The handle is a numerical handle with K latents: each keeps its own (mu_k, Sigma_k), optimiser moments, kept factor, alpha and
 * counters; the step counter t is shared.  One step, the estimator restated in its intended form:
 *     f_sk = mu_f,ik + sqrt(max(var_f,ik, 0)) eps_sk ,  s = 1 .. nMC          eps: ONE nMC x K table per step, shared by every point of
 *                                                                             the batch (grad_expectations!, MCVI.jl:93-107)
 *     ell_i = (1 / nMC) sum_s log p(c_i | f_s) ;  g_ik = (1 / nMC) sum_s d log p / d f_k ;  h_ik = (1 / nMC) sum_s d2 log p / d f_k^2
 *     grad_E_mu = g ,  grad_E_Sigma = h / 2                                   (numericalVI.jl:98-99 with nu = -g, lambda = h)
 *   and every latent k then takes exactly the step of NUMERICAL INFERENCE with (g_.k, h_.k), its own alpha_k included
 *   (numericalVI.jl:158-179 maps over the latents).  ELBO = rho sum_i ell_i - sum_k GaussianKL_k.
 *   The closed forms grad_samples! reduces to, with c the class of the point and y its one-hot vector:
 *     SoftMax          s = softmax(f):  log p = f_c - logsumexp(f) ;  d_k = y_k - s_k ;  d2_k = -s_k (1 - s_k)
 *     LogisticSoftMax  sg_k = logistic(f_k), s_k = sg_k / sum_j sg_j:  log p = log sg_c - log sum_j sg_j ;
 *                      d_k = (1 - sg_k)(y_k - s_k) ;  d2_k = (1 - sg_k) [-sg_k (y_k - s_k) - s_k (1 - s_k)(1 - sg_k)]
 *   evaluated stably: logsumexp subtracts the maximum, log sg(f) = -softplus(-f) (and log s_c = -log1p(sum of the others / sg_c)
 *   where c is the largest entry), 1 - sg(f) = sg(-f), and 1 - s_k of the largest
 *   entry is the sum of the OTHER entries over the total (the first maximum counts as the largest), so that ell, g, h keep their
 *   relative accuracy where a class probability approaches one (|mu| = 30, var = 0).
 *   clipping of the reference's MCIntegrationVI object is stored there and read by no MC code: it does not reach this library.
 * RANDOM STREAMS, continued (streams 0 and 1 keep their Gibbs meaning):
 *   eps_sk of (seed, t, stream) is the Normal of block 0 -- two uniforms (a, b) of the Philox counter (c0, c1, c2, c3) =
 *   (s K + k, t, stream, 0), key = seed, value sqrt(-2 log a) cos(2 pi b) -- with
 *     stream 2   the gradient draw of step t; t = 1, 2, ... is the step number, which is also ADAM's t
 *     stream 3   the draw of an ELBO evaluated after t steps (t = 0 before the first): repeated evaluations of an unchanged model agree
 *   On these two streams log and cos are not the device's math library but the following double arithmetic, one IEEE operation per
 *   written operation and no contraction, so that a host program reproduces the table bit for bit (tests/_mcvi_ref.py does):
 *     log a:  a = m 2^e (frexp), and m < 0.7071067811865476: m = 2 m, e = e - 1;  q = (m - 1) / (m + 1), z = q q,
 *             P = 1/23; for d = 21, 19, ..., 3, 1: P = P z + 1/d;  log a = e 0.6931471805599453 + (2 q) P
 *     cos 2 pi b:  r = b > 1/2 ? 1 - b : b;  r > 1/4: r = 1/2 - r and the sign flips;  r > 1/8: x = 6.283185307179586 (1/4 - r),
 *             z = x x, P = 1/17!; P = P z - 1/15!; P = P z + 1/13!; ... ; P = P z + 1; value x P (the sine series);  else
 *             x = 6.283185307179586 r, z = x x, P = 1/16!; P = P z - 1/14!; ... ; P = P z + 1 (the cosine series)
 * agp_svgp_mcvi_configure installs nMC (1 <= nMC <= 65536), the seed, natural != 0 for the natural gradient, and the optimiser, with
 *   the argument checks of agp_svgp_nvi_configure.  It is refused (AGP_ERR_UNSUPPORTED) on a handle without AGP_FLAG_MC, as
 *   agp_svgp_nvi_configure is on one with it; agp_svgp_nvi_step before it is AGP_ERR_INVALID.
 * On such a handle the entry points of NUMERICAL INFERENCE keep their meaning, with
 *   nvi_step        y int32[N]: the 0-based class index, read at idx (the form the LogisticSoftMax CAVI step takes); an index
 *                   outside [0, K) is latched and reported by agp_svgp_check_status as AGP_ERR_LABELS
 *   nvi_info / nvi_state / get_state / set_state    latent in [0, K) (else AGP_ERR_INVALID); t of nvi_state is the shared counter
 *   elbo            stream 3 at the handle's t
 *   predict_f       T[K][n_t];  predict_y  int32 argmax_k mu_f,k (the first maximum);  proba_y  out0 T[n_t][K], the link at the mean
 *                   (multiclass.jl:96-117): softmax(mu_f) / the normalised logistic; out1 is not written
 * agp_mc_normals writes the table double[nMC][K] of (seed, t, stream) to device memory (0 <= t < 2^32, nMC K < 2^32).
 * agp_mc_expectations is the expectation kernel on caller-supplied moments outside any model: lik->kind one of the two likelihoods,
 *   K = lik->n_class in [2, 64], y_class int32[n_pts] (0-based), mu, var, g, h double[K][n_pts], ell double[n_pts], all device;
 *   synchronises; a class index outside [0, K): AGP_ERR_LABELS.
 * The kernel: one wave per point, the lanes of a wave are (draw, latent) pairs -- 64 / P draws at a time, P the power of two >= K --
 *   so max and sum over k are P-lane butterflies and every lane owns one accumulator of g_k and h_k; the table is staged through
 *   LDS in tiles of 2048 doubles shared by the 4 points of a workgroup.  The order of summation is fixed by (nMC, K) alone. */
agp_status agp_svgp_mcvi_configure(agp_svgp* h, int32_t nMC, uint64_t seed, int32_t natural, int32_t opt_kind, double eta, double p1,
                                   double p2, double eps);
agp_status agp_mc_normals(agp_ctx* ctx, uint64_t seed, int64_t t, int32_t stream, int32_t nMC, int32_t K, void* out);
agp_status agp_mc_expectations(agp_ctx* ctx, const agp_lik_desc* lik, const void* y_class, const void* mu, const void* var,
                               int64_t n_pts, int32_t K, int32_t nMC, uint64_t seed, int64_t t, int32_t stream, void* ell, void* g,
                               void* h);

/* ---- PATHWISE SAMPLING (function draws from a trained posterior: SVGP, VGP with AnalyticVI / AnalyticSVI, exact GP) -----------------
 * Decoupled sampling (Wilson, Borovitskiy, Terenin, Mostowsky, Deisenroth 2020, "Efficiently sampling functions from Gaussian
 * process posteriors"): a prior function from l = n_features random Fourier features, a draw u ~ q(u), and Matheron's correction.
 * A draw is then an ordinary function: agp_pathwise_eval evaluates its S = n_samples paths at any number of test points in
 * O(n_t (l + m) S), streamed, with no n_t x n_t object (agp_svgp_predict_f_cov stops at n_t = 8192).
 * The draw is a SNAPSHOT object of its own: it copies what it needs from the handle (Z, the scales, the kernel kind and variance,
 * and the tables below), so training steps, set_kernel or destroying the handle afterwards neither change nor invalidate it.  It
 * keeps using the handle's context, which must outlive it.  Float64 device pointers throughout; the Layout rules above hold.
 * Per latent, with r = ||s o (x - x')|| and sigma2 the kernel variance:
 *   features   phi_j(x) = sqrt(2 sigma2 / l) cos(omega_j' (s o x) + p_j), p_j = 2 pi u_j; the frequencies and phases are shared by
 *              the S samples of a draw.  SqExponential: omega_j = z_j.  Matern52, Matern32, Exponential (nu = 5/2, 3/2, 1/2):
 *              omega_j = z_j sqrt(nu / G_j), G_j ~ Gamma(nu, 1) without rejection as G_j = n_j^2 / 2 + sum_{k < K} (-log u_jk),
 *              K = 2, 1, 0.  Then E[phi(x)' phi(x')] = sigma2 k(r) for the four kernels (checked by tests/test_pathwise_host.py).
 *   SVGP, VGP  U = mu 1' + Xa' E with Xa = chol_lower(-2 eta2)^-1 (Sigma = Xa' Xa: the square root of the Gibbs contract),
 *              V = K^-1 (U - Phi(Z) W), K = k(Z, Z) + jitt I as the handle holds it (VGP: Z = X)
 *   exact GP   V = alpha 1' - Sigma_y^-1 (Phi(X) W + sigma E), Sigma_y = K + sigma2_noise I and alpha as the handle holds them, sigma =
 *              sqrt(sigma2_noise) (needs a step or a refresh_K with targets before it: AGP_ERR_INVALID otherwise)
 *   paths      f_s(x) = sum_j phi_j(x) W_js + sum_r k(x, Z_r) V_rs
 * Given the features, f has mean k* K^-1 mu -- predict_f's mean exactly -- and covariance G G' + k* K^-1 Sigma K^-1 k*' with
 * G = Phi(x) - k* K^-1 Phi(Z) (exact GP: G G' + sigma2_noise k* Sigma_y^-2 k*', G = Phi(x) - k* Sigma_y^-1 Phi(X)).  As l grows this
 * tends to the matrix of agp_svgp_predict_f_cov without its + jitt I, up to O(jitt).  The feature error is O(1 / sqrt(l)) and is
 * NOT bounded here: at l = 512 one draw was 7 % off in covariance on a small case.
 * RANDOM STREAMS, continued (streams 0 - 3 keep their meaning): key = seed, t the CALLER's draw counter, 0 <= t < 2^32, and
 * s0 = 4 + 8 latent.  Normal = the Normal of block 0 with the log / cos 2 pi arithmetic contracted for streams 2 - 3; uniform k =
 * the k-th uniform of the stream (two per block).  Every sqrt and division is one IEEE operation, nothing is contracted, so
 * Omega, the phases, W and E are reproducible bit for bit on the host (tests/_pathwise_ref.py):
 *     z_jd   (j D + d, t, s0,     0)  Normal                  n_j   (j, t, s0 + 1, 0)  Normal
 *     u_jk   (j, t, s0 + 1, 1)        uniforms 2, 3 (k = 0, 1)      u_j   (j, t, s0 + 2, 0)  uniform 0;  p_j = 6.283185307179586 u_j
 *     W_js   (j S + s, t, s0 + 3, 0)  Normal                  E_is  (i S + s, t, s0 + 4, 0)  Normal
 *     G_j = (n_j n_j) 0.5, then G_j = G_j - log u_jk for k = 0 .. K - 1;  omega_jd = z_jd sqrt(nu / G_j)
 * agp_svgp_pathwise_draw  makes the draw (synchronises: it refreshes K and factors -2 eta2 once per latent).  A handle with an online
 *   prior is an ordinary sparse handle; multi-latent single-output likelihoods (LogisticSoftMax, Heteroscedastic) get one
 *   independent draw per latent.  AGP_ERR_UNSUPPORTED, touching nothing, by name: AGP_F32 handles; multi-output handles (MOSVGP,
 *   MOVGP); AGP_FLAG_SAMPLED; AGP_FLAG_NUMERICAL with or without AGP_FLAG_MC (a follow-up: the factor of Sigma is already kept
 *   there); latent-sharded and batch-sharded handles.  AGP_ERR_INVALID with a message: n_features or n_samples outside
 *   [1, 65536]; l D, l S or m S not below 2^32; t outside [0, 2^32); out = NULL.
 * agp_pathwise_eval  out[latent][s][i] at out + (latent * n_samples + s) * ldo + i, ldo >= n_t, ldx >= D; n_t = 0 is a successful
 *   no-op.  Test points go through the workspace [Phi(x) | k(x, Z)] in chunks of at most 4096, fewer where a chunk's share of the
 *   workspace -- 8 (l + m + S) bytes per point, all three rounded up to 64 -- would exceed AGP_PATHWISE_WS_BYTES (but at least
 *   64): one gemm_nt against the stored [W' | V'] gives both terms.  Asynchronous on the context's stream.
 * agp_pathwise_eval_grad  the input gradients of the paths, g_out[latent][s][i][d] = d f_s / d x_d (x_i) at g_out + ((latent *
 *   n_samples + s) * lds + i) * ldg + d, lds >= n_t, ldg >= D (padding never read or written).  A draw is a closed-form function, so
 *   is its gradient: with t_ird = s_d (x_id - Z_rd), q_ir = sum_d t_ird^2 and c_ir = sigma2 phi'(q_ir) (kernel_dbase of agp_hyper.h:
 *   the forms that are finite at r = 0 and never divide by r), per latent
 *       d f_s / d x_d (x_i) = - s_d sum_j amp sin(omega_j' (s o x_i) + p_j) omega_jd W_js  +  2 s_d sum_r c_ir t_ird V_rs ,
 *   amp = sqrt(2 sigma2 / l).  A test point that coincides with an inducing point is an ordinary input: t = 0 there exactly and the
 *   term adds exactly 0.  f_out (nullable): the values, laid out as agp_pathwise_eval writes them (ldo >= n_t) and bit for bit what
 *   it writes for the same arguments (the same kernels on the same chunk).  Nothing is drawn: the random streams are untouched.
 *   Chunks as agp_pathwise_eval; per chunk and latent the base workspace [A | C] (A_ij = -amp sin(.), C = c, q summed in ascending
 *   d from direct differences of the scaled coordinates: no cancellation far from the origin), then per dimension d one
 *   element-wise pass [A_ij s_d omega_jd | 2 s_d C_ir t_ird] into a second workspace of the same size and the evaluation's own
 *   gemm_nt against [W' | V']; the slabs of up to 64 dimensions (fewer where they would exceed AGP_PATHWISE_WS_BYTES) are staged and
 *   transposed into the caller's rows.  The second workspace and the staging are allocated by the first gradient call and belong
 *   to the draw.  No atomics, every sum in a fixed order: the same bits on every call.  The kernels written for it give a point
 *   the same bits wherever it stands in the call; gemm_nt does as long as it picks one kernel for every chunk size, which it does
 *   up to 1100 tiles of 64 x 64 per product, that is for n_samples <= 1088 (beyond, a point's row may move by rounding).  No
 *   limit on D beyond the draw's own.  n_t = 0 is a successful no-op; asynchronous on the context's stream.  AGP_ERR_UNSUPPORTED,
 *   touching no output: a latent of the draw has the ExponentialKernel ("ExponentialKernel is not differentiable at zero distance":
 *   its paths have a kink on Z; agp_svgp_predict_f_grad refuses it the same way).  AGP_ERR_INVALID with a message: xt or g_out NULL,
 *   n_t < 0, ldx < D, lds < n_t, ldg < D, ldo < n_t with f_out given.
 * agp_pathwise_maximize  multi-start ADAM ascent of the paths of one latent, on the device and in one launch: what Thompson sampling
 *   does with a draw.  A particle is a pair (sample s, start r), s < n_samples, r < n_starts; it starts at x0[s][r] (x0_shared: at
 *   x0[r], the same starts for every sample) clipped into the box [lo, hi] and takes T = steps steps, k = 1 .. T, with the f and
 *   d f_s / d x of agp_pathwise_eval_grad (the same closed forms, q summed over ascending d from direct differences):
 *       g = sign grad f_s(x)   (sign = +1, or -1 with minimize)
 *       m = beta1 m + (1 - beta1) g ;  v = beta2 v + (1 - beta2) g o g ;  mh = m / (1 - b1) ;  vh = v / (1 - b2)
 *       x = min(max(x + lr o mh / (sqrt(vh) + eps), lo), hi)
 *   m = v = 0 before step 1; b1 = beta1^k and b2 = beta2^k as running products (b = 1 before step 1, b = b beta per step).  After
 *   step T the path is evaluated once more: f_out is f_s of the returned x, and the FINAL iterate is returned, not the best one
 *   along the way, so every output is a continuous function of the inputs.  steps = 0 returns the clipped starts and their values.
 *   Outputs, each nullable (not all): x_out[s][r][d] at x_out + (s * n_starts + r) * ldxo + d; f_out[s][r] at f_out + s * ldf + r;
 *   per sample the best start -- the largest sign f, ties to the smallest r, a NaN never wins and start 0 does if every value is
 *   NaN -- as best_x[s][d] at best_x + s * ldb + d, best_f[s] (f itself, not sign f) and best_idx[s] (int64).  Padding is never
 *   read or written.  lo, hi and lr (D each, in input units) are HOST arrays, validated without a synchronisation and handed to
 *   the kernel with its arguments.  One workgroup carries a tile of particles through all T steps with x, m, v and the gradient
 *   in registers and Omega / s o Z staged through LDS; no atomics, no communication between workgroups, every sum over j, then
 *   r, ascending in one accumulator: a particle has the same bits wherever it stands in the call, whichever particles share its
 *   tile, with x0 shared or per sample, and on every repeat.  The particle state (n_samples n_starts (D + 1) doubles) belongs to
 *   the draw and is allocated by the first call; a call with more particles than any before re-allocates it (the only place that
 *   may wait for the device).  Asynchronous on the context's stream; nothing is drawn; the draw is a snapshot as for the other
 *   calls.  AGP_ERR_UNSUPPORTED, touching no output: the latent has the ExponentialKernel ("ExponentialKernel is not
 *   differentiable at zero distance"); D > 64 ("D > 64 is not supported").  AGP_ERR_INVALID with a message: p, x0 or opts NULL; all
 *   five outputs NULL; latent outside [0, n_latent); n_starts < 1 or n_samples n_starts >= 2^31; ldx0 < D, ldxo < D, ldf <
 *   n_starts, ldb < D (of outputs that are given); steps outside [0, 65536]; beta1 or beta2 outside [0, 1); eps not finite and
 *   positive; lo_host, hi_host or lr_host NULL, a non-finite bound, lo > hi, a step size that is not finite and positive.
 * agp_pathwise_get   which = AGP_PW_OMEGA (l x D, ld >= D), AGP_PW_PHASE (l; ld not read), AGP_PW_W (l x S, ld >= S), AGP_PW_V
 *   (m x S, ld >= S), AGP_PW_E (m x S, ld >= S).
 * agp_pathwise_features  the spectral draw alone, outside any model: omega_out double[l][D], phase_out double[l], dense, device;
 *   of the kernel only the kind is read (the scales enter at evaluation); latent >= 0 selects s0.  Synchronises. */
enum { AGP_PW_OMEGA = 0, AGP_PW_PHASE = 1, AGP_PW_W = 2, AGP_PW_V = 3, AGP_PW_E = 4 };
enum { AGP_PATHWISE_WS_BYTES = 64 * 1024 * 1024 };
typedef struct agp_pathwise agp_pathwise;
agp_status agp_svgp_pathwise_draw(agp_svgp* h, int32_t n_features, int32_t n_samples, uint64_t seed, int64_t t, agp_pathwise** out);
agp_status agp_pathwise_eval(agp_pathwise* p, const void* xt, int64_t ldx, int64_t n_t, void* out, int64_t ldo);
agp_status agp_pathwise_eval_grad(agp_pathwise* p, const void* xt, int64_t ldx, int64_t n_t,
                                  void* f_out, int64_t ldo, /* nullable: the values, laid out as agp_pathwise_eval writes them */
                                  void* g_out, int64_t lds, int64_t ldg);
typedef struct {
  int32_t steps;            /* T, 0 <= T <= 65536; T = 0 returns the clipped starts and their values */
  int32_t minimize;         /* 0: ascend, 1: descend */
  int32_t x0_shared;        /* 0: x0[s][r][d] at x0 + (s * n_starts + r) * ldx0 + d;  1: x0[r][d], the same starts for every sample */
  double beta1, beta2, eps; /* 0 <= beta < 1, eps > 0 */
  const double* lo_host;    /* D lower bounds, host memory (like ard_scales_host), finite, lo <= hi */
  const double* hi_host;
  const double* lr_host;    /* D step sizes in input units, host memory, finite and > 0 */
} agp_pw_ascent_opts;
agp_status agp_pathwise_maximize(agp_pathwise* p, int32_t latent, const void* x0, int64_t ldx0, int64_t n_starts,
                                 const agp_pw_ascent_opts* opts,
                                 void* x_out, int64_t ldxo, /* nullable: [s][r][d], ldxo >= D */
                                 void* f_out, int64_t ldf,  /* nullable: [s][r], ldf >= n_starts */
                                 void* best_x, int64_t ldb, /* nullable: [s][d], ldb >= D */
                                 void* best_f,              /* nullable: [s] */
                                 void* best_idx);           /* nullable: int64 [s] */
/* "ACQUISITION FUNCTIONS": the same ascent on an acquisition function of the handle's predictive moments */
agp_status agp_svgp_acq_maximize(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* x0, int64_t ldx0, int64_t n_starts,
                                 const agp_pw_ascent_opts* opts,
                                 void* x_out, int64_t ldxo, /* nullable: [r][d], ldxo >= D */
                                 void* a_out,               /* nullable: [r] */
                                 void* best_x,              /* nullable: [d], D values */
                                 void* best_a,              /* nullable: one double */
                                 void* best_idx);           /* nullable: one int64 */
/* "ACQUISITION FUNCTIONS", paragraph "Pending points" */
agp_status agp_svgp_acquisition_pending(agp_svgp* h, int32_t latent, const agp_acq_desc* desc,
                                        const void* xp, int64_t ldp, int64_t n_pending, double noise,
                                        const void* xt, int64_t ldx, int64_t n_t,
                                        void* alpha_out, void* grad_out /* nullable */, int64_t ldg);
agp_status agp_svgp_acq_maximize_batch(agp_svgp* h, int32_t latent, const agp_acq_desc* desc,
                                       const void* xp /* nullable iff n_pending == 0 */, int64_t ldp, int64_t n_pending, double noise,
                                       int64_t q, const void* x0, int64_t ldx0, int64_t n_starts, const agp_pw_ascent_opts* opts,
                                       void* xb_out /* [q][ldxb] */, int64_t ldxb,
                                       void* ab_out /* double[q], nullable */, void* idxb_out /* int64[q], nullable */);
/* "ACQUISITION FUNCTIONS", paragraph "Joint batches" */
agp_status agp_svgp_acquisition_joint(agp_svgp* h, int32_t latent, const agp_acq_desc* desc,
                                      const void* xp /* nullable iff n_pending == 0 */, int64_t ldp, int64_t n_pending, int64_t q,
                                      const void* xq, int64_t ldx, int64_t n_sets,
                                      const void* eps /* double [S][lde] */, int64_t lde, int64_t S,
                                      void* alpha_out, void* grad_out /* nullable */, int64_t ldg);
agp_status agp_svgp_acq_maximize_joint(agp_svgp* h, int32_t latent, const agp_acq_desc* desc,
                                       const void* xp /* nullable iff n_pending == 0 */, int64_t ldp, int64_t n_pending, int64_t q,
                                       const void* x0, int64_t ldx0, int64_t n_starts,
                                       const void* eps /* double [S][lde] */, int64_t lde, int64_t S, const agp_pw_ascent_opts* opts,
                                       void* x_out, int64_t ldxo, /* nullable: [r][j][d], ldxo >= D */
                                       void* a_out,               /* nullable: [r] */
                                       void* best_x, int64_t ldb, /* nullable: [j][d], ldb >= D */
                                       void* best_a,              /* nullable: one double */
                                       void* best_idx);           /* nullable: one int64 */
agp_status agp_pathwise_info(agp_pathwise* p, int32_t* n_latent, int32_t* n_features, int32_t* n_samples, int64_t* m, int64_t* D);
agp_status agp_pathwise_get(agp_pathwise* p, int32_t latent, int32_t which, void* out, int64_t ld);
agp_status agp_pathwise_destroy(agp_pathwise* p);
agp_status agp_pathwise_features(agp_ctx* ctx, const agp_kernel_desc* k, int64_t D, int32_t n_features, uint64_t seed, int64_t t,
                                 int32_t latent, void* omega_out, void* phase_out);

/* ---- multi-GPU: one process per GPU, collectives behind the ABI --------------------------------
 * The path shards in two ways and both reduce to in-place SUM all-reduces of library-owned device buffers:
 *   AGP_SHARD_LATENT : this handle holds the latent slice [latent_offset, latent_offset + n_latent) of the model, every rank
 *                      sees the same minibatch.  LogisticSoftMax: sum_k gamma_k (a B-vector) twice per step
 *                      (src/likelihood/logisticsoftmax.jl:65-72); latent-sharded multi-output: the (mean_f, var_f) exchange
 *                      buffer once per step (src/models/single_and_multi_output_utils.jl:24-84); otherwise no collective.
 *   AGP_SHARD_BATCH  : every rank holds all latents and sees ITS SHARE of the minibatch (idx, B are the local share,
 *                      rho = N / B_total); the batch statistics [kappa'(rho g1) | rho kappa' diag(g2) kappa] (one triangle,
 *                      packed as 64x64 tiles: mp + nt(nt+1)/2 * 4096 elements per latent, 4.46 MB at m = 1024 f64) are
 *                      all-reduced once per step (src/inference/analyticVI.jl:168,179), then every rank applies the identical
 *                      global step.
 * agp_comm_unique_id : rank 0 draws the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks over whatever host
 *                      channel exists (MPI, a file, Julia's Distributed, torch.distributed's store).
 * agp_comm_init      : ncclCommInitRank on ctx's device; collectives are enqueued on ctx's stream (RCCL over xGMI).
 * agp_comm_init_callback : the host supplies the all-reduce instead (must sum `count` elements of `dtype` in place at the
 *                      DEVICE pointer `buf`, ordered after the work already enqueued on `hip_stream`; return 0 on success).
 *                      `hip_stream` is the ctx's stream, or -- AGP_SPLIT_OVERLAP=1 -- a stream of the communicator's own.
 * AGP_SPLIT_OVERLAP=1 (environment, default off, read at every step; batch-parallel single-latent steps that ride on the task-graph
 *                      launches): the statistics are all-reduced as AGP_SPLIT_OVERLAP_GROUPS (default 4) contiguous ranges -- groups
 *                      of block columns -- one after the other on the communicator's own stream, and the next step's factorisation
 *                      starts on the first group while the others travel (its tile workgroups wait for their column's group).
 *                      Same results bit for bit; every rank must use the same setting (the call sequence differs).
 * All ranks must issue the same sequence of *_multi calls. */
typedef struct agp_comm agp_comm;
enum { AGP_COMM_ID_BYTES = 128 };
enum { AGP_SHARD_LATENT = 0, AGP_SHARD_BATCH = 1 };
typedef int32_t (*agp_allreduce_fn)(void* user, void* buf, int64_t count, int32_t dtype, void* hip_stream);
agp_status agp_comm_unique_id(uint8_t* id_host /* [AGP_COMM_ID_BYTES] */);
agp_status agp_comm_init(agp_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id_host, agp_comm** out);
agp_status agp_comm_init_callback(agp_ctx* ctx, int32_t rank, int32_t world, agp_allreduce_fn fn, void* user,
                                  agp_comm** out);
agp_status agp_comm_destroy(agp_comm* comm);
agp_status agp_comm_info(agp_comm* comm, int32_t* rank_host, int32_t* world_host, int32_t* is_rccl_host);
/* sum all-reduce of a device buffer in place on the ctx stream (what the *_multi calls use; exposed for host drivers) */
agp_status agp_comm_allreduce(agp_comm* comm, void* buf, int64_t count, int32_t dtype);
/* accounting since the last read: number of collectives, bytes reduced (per rank), and -- when timing was enabled with
 * agp_comm_timing(comm, n) -- their summed duration from HIP events on the ctx stream (synchronises).  n = 1 brackets every
 * collective, n > 1 every n-th one (the two event records cost the stream ~20 us each time); the sum is scaled to all calls. */
agp_status agp_comm_timing(agp_comm* comm, int32_t on);
agp_status agp_comm_stats(agp_comm* comm, int64_t* n_calls_host, int64_t* bytes_host, double* ms_host);
/* Diagnostic (one-GPU boxes): a stand-in for an xGMI ring all-reduce that occupies the chip the way RCCL's ring kernel does -- n_wg
 * workgroups of n_threads that must ALL be resident to finish (grid barrier, the buffer moved through their registers, grid
 * barrier), lasting at least min_us.  Sum over one rank: the buffer keeps its values.  Enqueued on `stream` (a hipStream_t; the
 * stream an agp_allreduce_fn callback is handed).  stuck_dev (nullable, device int32): incremented by every workgroup whose bounded
 * wait for the others ran out (~1 s) -- the stand-in then gives up instead of hanging the device.  One n_wg per process. */
agp_status agp_comm_standin_allreduce(void* buf, int64_t count, int32_t dtype, void* stream, int32_t n_wg, int32_t n_threads,
                                      double min_us, int32_t* stuck_dev);

/* update_parameters!(model, state, x, y) (src/training/training.jl:140-158) of a sharded model: agp_svgp_cavi_step with the
 * exchange points above carried out on `comm`.  comm == NULL or world == 1 degenerates to the single-GPU step through the
 * same phase sequence (a handle that owns only a slice of a multi-output model's latents refuses comm == NULL).
 * Poisson / Heteroscedastic likelihoods (AGP_SHARD_BATCH only; the two heteroscedastic latents are coupled point-wise and share a
 * handle): lambda is re-estimated from sums over the WHOLE minibatch (poisson.jl:78, heteroscedastic.jl:94) -- three doubles
 * [S0, S1, B_local] are all-reduced between the local update's partial sums and its finish.
 * Scheduling note (round 3, invisible through the ABI, like agp_svgp_cavi_step's): a single-latent AGP_SHARD_BATCH step over several
 * ranks in a training loop (next minibatch announced with agp_svgp_prefetch) leaves its eta step PENDING on the all-reduced
 * statistics; the next step's factorisation launch takes it as its prologue.  Every other entry point completes it first. */
agp_status agp_svgp_cavi_step_multi(agp_svgp* h, agp_comm* comm, int32_t mode, const void* x, int64_t ldx, const void* y,
                                    const int64_t* idx, int64_t B, double rho);
/* ELBO(model, state, y) of the last minibatch of a sharded run, identical on every rank (analyticVI.jl:255-297):
 * latent mode sums the ranks' shares (shared per-point terms are counted by the owner of latent 0); batch mode sums the data
 * and augmented-KL terms of the shards and counts the replicated Gaussian KL once (rank and world of the shard are taken from
 * the communicator). */
agp_status agp_svgp_elbo_multi(agp_svgp* h, agp_comm* comm, int32_t mode, double* elbo_host);
/* update_hyperparameters! (src/hyperparameter/autotuning.jl:86-140) of a sharded model.
 *   tied = 0 : every latent optimises its own kernel and Z (the reference's deep copies, latentgp.jl:63-68).  Latent-sharded: no
 *              collective, except that a sharded multi-output model first re-exchanges mean_f under the updated posterior.
 *              Batch-sharded (the handle has seen a batch-mode call or agp_svgp_set_batch_shard): per latent, the gradient
 *              (1 + D + m*D doubles; data part summed over the shards, Gaussian-KL part weighted 1 / world) is all-reduced and
 *              every rank takes the identical ADAM step -- the replicas stay bit-identical.
 *   tied = 1 : ONE kernel and ONE Z shared by all latents (an opt-in extension; BASELINE.json config 4's "all-reduce on the
 *              Z hyper-grad"): the gradients of the local latents are summed, all-reduced (1 + D + m*D doubles), and the same
 *              ADAM step is applied to every latent on every rank. */
agp_status agp_svgp_hyper_step_multi(agp_svgp* h, agp_comm* comm, int32_t tied);
/* predict_f / predict_y / proba_y of a latent-sharded multi-output model: partial mixes all-reduced (n_task x n_t each), the
 * task likelihoods finished in place.  what: 0 predict_f (mu_out, var_out nullable), 1 predict_y (mu_out), 2 proba_y
 * (mu_out, var_out; Gauss-Hermite rule as in agp_svgp_proba_y).  Outputs T[n_task][n_t]. */
agp_status agp_svgp_predict_multi(agp_svgp* h, agp_comm* comm, int32_t what, const void* xt, int64_t ldx, int64_t n_t,
                                  void* mu_out, void* var_out, const double* gh_nodes_host, const double* gh_weights_host,
                                  int32_t n_nodes);

#ifdef __cplusplus
}
#endif
#endif /* AGP_HIP_H */
