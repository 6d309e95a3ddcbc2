// agp_capi.hip -- C ABI of libagp_hip.so (see include/agp_hip.h).  Host-side orchestration of the gfx950 kernels in
// agp_linalg.h / agp_cavi.h: one process per GPU, everything enqueued on the caller's HIP stream.  This file holds the model
// classes (Svgp<T> and the six derived from it) and the extern "C" surface, and is the one translation unit: it includes the kernel
// headers, then agp_ctx.h (context, error macros), agp_chol_host.h (Cholesky driver) and agp_blas_host.h (GEMM / SYRK / kernel-matrix
// launchers), then agp_svgp_base.h (the handle interface) and the host drivers of the other subjects (agp_lpd_host.h,
// agp_pathwise_host.h, agp_acq_host.h, agp_acq_joint_host.h, agp_blocks_host.h, agp_select_host.h, agp_comm_host.h), each where its
// text stood.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "agp_cavi.h"
#include "agp_elbo_stream.h"
#include "agp_comm.h"
#include "agp_hyper.h"
#include "agp_kmeans.h"
#include "agp_greedy.h"
#include "agp_linalg.h"
#include "agp_nvi.h"
#include "agp_rand.h"
#include "agp_pathwise.h"
#include "agp_lpd.h"
#include "agp_predgrad.h"
#include "agp_acq.h"
#include "agp_acq_batch.h"
// (the host layers after every kernel header, as they stood in this file: the order of the kernels in the code object is kept)
#include "agp_ctx.h"
#include "agp_chol_host.h"
#include "agp_blas_host.h"

// (the handle interface and the other host drivers, here and further down: each where its first use of a kernel template must come)
#include "agp_lpd_host.h"
#include "agp_svgp_base.h"
#include "agp_pathwise_host.h"
#include "agp_acq_host.h"
#include "agp_acq_joint_host.h"
template <typename T>
struct Svgp : SvgpBase {
  struct Latent {
    KernelHost k;
    T* scales = nullptr;  // device, D
    T* Z = nullptr;       // m x D
    T *Zsc = nullptr, *zn = nullptr;  // scaled, tile-padded copy of Z (mp x Dp) and its squared norms: the Y side of the MFMA
    bool zsc_valid = false;           // kernel matrix (k_scale_rows); redone when Z or the scales change
    T* L = nullptr;       // mp x mp : K then chol(K) (lower)
    T* Xk = nullptr;      // L^-1
    T* Kinv = nullptr;
    T* mu0 = nullptr;
    T* kinv_mu0 = nullptr;
    T* eta1 = nullptr;
    T* eta2 = nullptr;
    T* La = nullptr;      // -2*eta2 then its Cholesky factor
    T* Xa = nullptr;      // La^-1   (Sigma = Xa' Xa)
    T* v = nullptr;       // Xa eta1 (mu = Xa' v)
    T* Sigma = nullptr;
    T* mu = nullptr;
    T* Knm = nullptr;
    T* kappa = nullptr;
    T* Wbuf = nullptr;    // (Bp + 64) x mp : [kappa ; eta1'] -> [W ; v'] by the augmented Cholesky
    T* pk = nullptr;      // K~ partial slices of this latent [2*mp/64][ldp]
    T *Knm_alt = nullptr, *kappa_alt = nullptr, *Wbuf_alt = nullptr, *pk_alt = nullptr;  // prefetch targets
    T* kappa_old = nullptr;  // third kappa buffer: the minibatch whose natural-gradient step is still pending (see Pending)
    T* DgK = nullptr;     // diagonal 64x64 factors of chol(K)      (mp x 64)
    T* DgA = nullptr;     // diagonal 64x64 factors of chol(-2 eta2)
    T* Apred = nullptr;   // K^-1 - K^-1 Sigma K^-1
    // hyper-parameter iteration: C = kappa' diag(w) kappa + K^-1 / 4 of the natural-gradient step that the factorisation launch took
    // as its prologue (ProArgs::Cout); valid until the next local step / natural-gradient step (hypergrad, k_hyper_gK_fused)
    T* Cmat = nullptr;
    bool C_valid = false;
    const T* C_kap = nullptr;  // the kappa buffer it was formed from
    T* apred = nullptr;   // K^-1 mu
    bool K_stale = true, post_valid = false, pred_valid = false, predvar_valid = false, kappa_valid = false;
    bool kappa_eval = false;  // kappa / Knm / pk hold the kernel matrices of the last FRESH evaluation batch (ev_x ..., round 6)
    bool keep_last = false;  // this step reuses kappa / K~ of the previous full-batch step
    bool via_inverse = false;  // this step gets W, v from the available inverse factor instead of a new factorisation
    // hyper-parameter optimiser state (ADAM): kernel parameters on the host, Z on the device
    std::vector<double> k_m, k_v;  // (host staging of the moments for agp_svgp_hyper_opt_state; the live ones are kadam)
    int k_step = 0, z_step = 0;
    double* kadam = nullptr;       // device: ADAM moments of the kernel parameters [m (1 + D) | v (1 + D)]
    bool host_params_stale = false;  // the device parameter array moved (device ADAM): k.variance / k.scales lag behind
    double *z_am = nullptr, *z_av = nullptr;
    // La holds: 0 = -2*eta2 (unfactored), 1 = its Cholesky factor ; xa_valid: Xa = La^-1 is current
    int la_state = 0;
    bool xa_valid = false;
    // v = Xa eta1 formed by materialize() next to mu belongs to the inverse with this number (aug_factor counts them): a step that
    // takes W, v from the inverse uses it instead of launching the triangular mat-vec itself
    int64_t xa_epoch = 0, v_epoch = -1;
    int64_t sigma_epoch = -1;  // xa_epoch of the inverse whose Sigma = Xa' Xa the factorisation launch itself has left in Sigma (ProdArgs)
    bool v_ready = false;
    double half_logdetK = 0.0;
    bool logdet_pending = false;  // half_logdetK still sits in logdetK_dev (asynchronous K refresh)
    // AGP_FLAG_STALE_K: the step-side copies of (inv(K), L^-1, K\mu0, logdet K) frozen at the first hyper step of a train! --
    // what the reference keeps using until train! ends (training.jl:187-208); the members above are always the fresh ones
    T *sKinv = nullptr, *sXk = nullptr, *skinv_mu0 = nullptr;
    double s_half_logdetK = 0.0;
    bool stale_on = false;
    // OnlineSVGP streaming prior (onlinetraining.jl:170-180, latentgp.jl:217-237): the previous posterior enters through
    // Z_a, invD_a = Sigma_a^-1 - K_a^-1, eta1_a ; kappa_a = K_ab K^-1, K~_a = K_a - kappa_a K_ab'
    bool on = false, on_dirty = false, on_first = false;
    int64_t ma = 0, map = 0;
    T *Za = nullptr, *invDa = nullptr, *peta1 = nullptr, *kappa_a = nullptr, *Kab = nullptr, *Kta = nullptr, *onT = nullptr,
      *onQ = nullptr, *kinv_mu0_on = nullptr, *Kinv_on = nullptr, *ov0 = nullptr, *ov1 = nullptr, *oh1 = nullptr,
      *oh2 = nullptr, *oh3 = nullptr;
    double prevLa = 0.0;
  };
  std::vector<Latent> lat;
  int64_t m = 0, mp = 0, D = 0, Bmax = 0, Bp = 0;  // Bp = padded max batch
  int nl = 0;
  double jitter = 1e-4;
  LikParams<T> lp{};
  // shared batch buffers
  T *pw0 = nullptr, *pw1 = nullptr;  // row-statistic scratch [ldp]
  // hyper-parameter step (update_hyperparameters!, autotuning.jl:86-140)
  bool hy_k = false, hy_z = false;
  double hy_keta = 0.01, hy_zeta = 0.001, hy_b1 = 0.9, hy_b2 = 0.999, hy_eps = 1e-8;
  int hy_krule = AGP_OPT_ADAM, hy_zrule = AGP_OPT_ADAM;  // agp_svgp_hyper_rule: ADAM / Descent / Momentum (opt_rule_delta)
  double hy_krho = 0.0, hy_zrho = 0.0;
  T *hyKap = nullptr, *hyKnm = nullptr;  // kappa (Knm) under the fresh inv(K) (kernel) for the hyper-gradient, AGP_FLAG_STALE_K
  T* hy_pZ2 = nullptr;
  double *hy_pvar2 = nullptr, *hy_pscale2 = nullptr;
  T* hy_upart = nullptr;                 // two per tile row: partial column sums of kappa' g_mu (k_gemm_nt<EPI_HK> -> k_hyper_gK_fused)
  T *hyH1 = nullptr, *hyH2 = nullptr, *hyH3 = nullptr, *hy_gmu = nullptr, *hy_gs = nullptr, *hy_muf = nullptr,
    *hy_pZ = nullptr, *hy_dZ = nullptr;
  double *hy_pvar = nullptr, *hy_pscale = nullptr, *hy_g = nullptr;
  int64_t hy_tiles = 0;  // tiles that hy_pvar / hy_pscale hold partial sums for (hyper_alloc)
  // multi-output mode (MOSVGP): n_task likelihoods over A-mixed latents
  bool mo = false;
  MoCfg<T> mocfg{};
  int nT = 0;
  int64_t ystride = 0;
  T* A_dev = nullptr;
  double *gradA_dev = nullptr, *am_dev = nullptr, *av_dev = nullptr;
  int a_step = 0;
  double a_eta = 0, a_b1 = 0.9, a_b2 = 0.999, a_eps = 1e-8;
  T *mo_mixm = nullptr, *mo_mixv = nullptr, *mo_th = nullptr, *mo_cc = nullptr, *mo_th_save = nullptr;
  // latent-sharded multi-output model (one handle per GPU holds the latents [qlo, qlo + nl) of qtot): the mixing needs every
  // latent's (mean_f, var_f) on the batch, exchanged through `fall` = T[2][qtot][Bp] (own rows filled, the rest zero, so the
  // sum over ranks is the all-gather of SURVEY.md section 8e).  fall_state: 0 empty, 1 = pre-update values published by
  // step_local (-> mo_mix), 2 = current-posterior values published by mo_refresh_f (-> elbo / hypergrad), 3 = consumed.
  bool mo_sharded = false;
  int qtot = 0, qlo = 0, fall_state = 0;
  T* fall = nullptr;
  int Qa() const { return mo_sharded ? qtot : nl; }
  // prefetch of the next minibatch's Knm / kappa on a second stream (overlaps the latency-bound factorisation)
  hipStream_t pf_stream = nullptr;
  static constexpr int PF_SIDE = 3;  // further look-ahead streams of a handle with several latents (prefetch())
  hipStream_t pf_side[PF_SIDE] = {nullptr, nullptr, nullptr};
  hipEvent_t pf_fork = nullptr, pf_join[PF_SIDE] = {nullptr, nullptr, nullptr};
  hipEvent_t pf_done = nullptr, step_done[2] = {nullptr, nullptr};
  int step_parity = 0;
  bool pf_valid = false;
  // hand-over word with the look-ahead stream (DagSync): sig[0] = "started" (written by the step's task graph).  The release of
  // a step's kappa buffers -- what the NEXT look-ahead but one waits for -- is either an event recorded on the stream
  // (slot_kind 0) or, when the step after it starts with a task graph that stores its `started` number, that number (slot_kind
  // 1: nothing is enqueued on the stream).  Which one is only known when the next step is enqueued, hence rel_pending.
  // sig[1] = "look-ahead done" (round 3): written by a one-thread kernel behind the look-ahead's GEMM, polled by a one-wave kernel
  // at the head of the step that adopts the buffers -- the cross-stream event wait cost the step's queue ~6 us of idling
  int32_t* sig[2] = {nullptr, nullptr};
  int32_t pf_seq = 0;
  int sig_state = 0;  // 0 not tried, 1 usable, -1 not available / switched off (AGP_PF_INKERNEL=0)
  int32_t started_seq = 0;
  bool rel_pending = false;
  int rel_slot = 0, slot_kind[2] = {0, 0};
  int32_t slot_seq[2] = {0, 0};
  const void* pf_x = nullptr;
  const int64_t* pf_idx = nullptr;
  int64_t pf_B = 0, pf_ldx = 0;
  int64_t ldp = 0;
  T *Kt = nullptr, *muf = nullptr, *varf = nullptr, *cbuf = nullptr, *theta = nullptr, *gamma = nullptr,
    *rbuf = nullptr, *wbuf = nullptr;              // [nl][Bp]
  T *alpha = nullptr, *beta = nullptr, *gsum = nullptr, *alpha_save = nullptr;  // [Bp]
  T *emuf = nullptr, *evarf = nullptr;             // ELBO-time mean_f / var_f [nl][Bp]
  T* stats = nullptr;                              // [nl][mp + nt(nt+1)/2 * 64*64]: kappa' r, then the lower tiles of kappa' diag(w) kappa
  int64_t stats_stride() const { return mp + (mp / TILE) * (mp / TILE + 1) / 2 * TILE * TILE; }
  T* Tw = nullptr;                                 // mp x mp scratch
  T* Tw2 = nullptr;                                // mp x mp scratch (predict)
  int tw2_kis_of = -1;                             // latent whose K^-1 Sigma the scratch holds, -1: something else
  T* tmpv = nullptr;                               // mp
  T* lr_dev = nullptr;
  int32_t* info_dev = nullptr;   // failure latch of the factorisations of -2*eta2 (asynchronous steps)
  int32_t* infoK_dev = nullptr;  // ... and of K_ZZ (read where it is produced: refresh_K synchronises)
  int* flags_dev = nullptr;
  double* scal_dev = nullptr;                      // 16 doubles
  // prediction workspace
  T *Kstar = nullptr, *ppm = nullptr, *ppv = nullptr, *pmu = nullptr, *pvar = nullptr;
  int64_t pred_chunk = 0, pred_nt_cap = 0;
  double* gh_dev = nullptr;
  int gh_cap = 0, gh_n = 0;  // Gauss-Hermite nodes | weights (agp_svgp_set_quadrature / proba_y)
  T* lam_dev = nullptr;       // Poisson / heteroscedastic lambda (state re-estimated by every local update); Gaussian noise sigma2
                              // when it is optimised (LikParams::noise_dev)
  double* noise_adam = nullptr;
  double noise_eta = 0.0;
  double* lam_part = nullptr; // per-workgroup partial sums of the lambda update
  double* frob_part = nullptr;  // row partial sums of frob_dot
  int64_t frob_cap = 0;
  agp_status frob_dot(const T* A, const T* Bm, int64_t ld, int64_t n, double* out) {
    if (n > frob_cap) {
      if (frob_part) (void)hipFree(frob_part);
      frob_part = nullptr;
      frob_cap = 0;
      AGPCHK(dmalloc(ctx, &frob_part, n));
      frob_cap = n;
    }
    hipLaunchKernelGGL((k_frob_dot_rows<T>), dim3((unsigned)n), dim3(256), 0, st(), A, Bm, ld, n, frob_part);
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(1024), 0, st(), (const double*)frob_part, n, out);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  // The natural-gradient step of the last CAVI step, not taken yet: the next step's task-graph launch takes it as its prologue
  // (ProArgs, agp_chol.h) -- the 53 us symmetric product then no longer sits between two factorisation chains.  Everything else
  // that touches the posterior calls flush() first.  kap is the physical kappa buffer of that minibatch (it survives the rotation of
  // the look-ahead buffers: kappa has three of them).
  struct Pending {
    bool on = false;
    int64_t Bq = 0;
    T lr = T(0);
    const T* kap = nullptr;
    const T *Kinv = nullptr, *kinv_mu0 = nullptr;
    const T *r = nullptr, *w = nullptr;  // rho grad_E_mu / rho grad_E_Sigma of that minibatch (the r / w pair current at the time)
  } pend;
  // ... and the batch-parallel form of it (agp_svgp_cavi_step_multi, AGP_SHARD_BATCH over several ranks): the statistics have been
  // all-reduced into `stats` = [t | packed lower tiles]; the eta step from them rides on the next launch as well
  struct PendingPacked {
    bool on = false;
    T lr = T(0);
    const T *Kinv = nullptr, *kinv_mu0 = nullptr;
    // AGP_SPLIT_OVERLAP: the statistics are still arriving, group by group, on the communicator's stream (arrive words at `epoch`)
    bool overlap = false;
    int32_t epoch = 0;
    agp_comm* cm = nullptr;
  } pendp;
  // arrival words of the block-column groups (device memory, ARRIVE_STRIDE apart), the step counter they carry, the groups
  int32_t* arrive_dev = nullptr;
  int32_t arrive_epoch = 0;
  int ov_ng = 0;
  int64_t ov_nt = 0;
  int64_t ov_off[8] = {}, ov_cnt[8] = {};
  unsigned char ov_grp[32] = {};
  // Second (r, w) pair: a task-graph launch with the row-statistics EPILOGUE (EpiArgs) writes this step's r, w while late workgroups
  // of its own prologue may still read the previous step's -- the two pairs alternate.
  T *rbuf2 = nullptr, *wbuf2 = nullptr;
  // The launch behind such a task graph -- its in-stream fallback (k_chol_safe), which also redoes the rows if it has to run -- is
  // DEFERRED to the head of the next step, where it also carries that step's wait for its look-ahead: one tiny kernel between two
  // task graphs instead of two (k_safe_rowstats + k_wait_ge_fast; every kernel costs the in-order queue ~5 us).  Anything else that
  // needs the step's results runs it first (flush()).
  struct SafeDeferred {
    bool on = false;
    CholBatch<T> bt{};
    SafeSrc<T> src{};
    RowstatsBatch<T> rb{};
    int64_t ne = 0, nt = 0, B = 0;
    int ns = 0;
    T rho = T(0);
    const T* y = nullptr;
    const int64_t* idx = nullptr;
    T *r = nullptr, *w = nullptr;
    unsigned grid = 1;
    unsigned long long* trace = nullptr;  // (AGP_STEP_TRACE: the stamp record of the launch this one stands behind)
  } sdef;
  // The first tiles of the pending natural-gradient step's product, prepared by the deferred launch for the head of the next
  // task-graph launch (ProArgs::pre: partial tiles + a validity element); s00_for names the pending step they belong to (kappa, w)
  // -- only the launch that immediately follows uses them, every other consumer of the pending step computes as before
  T* s00buf = nullptr;
  struct {
    bool on = false;
    const T *kap = nullptr, *w = nullptr;
    int64_t K = 0;
  } s00_for;
  agp_status run_deferred_safe(const int32_t* pf_word = nullptr, int32_t pf_want = 0, bool want_s00 = false) {
    if (!sdef.on) return AGP_OK;
    sdef.on = false;
    s00_for.on = false;
    // (the pending step is this launch's own: w is the row statistics' output the fallback would redo)
    const bool s00 = pro_pre_on<T>() && want_s00 && pend.on && !pendp.on && pend.w == sdef.w && pend.Bq >= TILE && pend.Bq % TILE == 0;
    if (s00 && !s00buf) AGPCHK(dmalloc<T>(ctx, &s00buf, PRO_PRE_VALID + 16));
    hipLaunchKernelGGL((k_safe_rowstats<T>), dim3(sdef.grid), dim3(CHOL_THREADS), 0, st(), sdef.bt, sdef.src, mp, mp, mp, sdef.ne,
                       sdef.nt, info_dev, m, ctx->safe_bar, ctx->safe_retries, sdef.B, sdef.ns, sdef.rb, ldp, mp, mp, (T)jitter,
                       sdef.rho, lp, sdef.y, sdef.idx, Kt, muf, varf, cbuf, theta, sdef.r, sdef.w, flags_dev, (const T*)lam_dev,
                       gamma, 1, pf_word, pf_want, s00 ? pend.kap : nullptr, (int64_t)mp, s00 ? pend.Bq : 0,
                       s00 ? (const T*)pend.w : nullptr, s00 ? s00buf : nullptr, sdef.trace);
    LAUNCHCHK(ctx);
    if (s00) {
      s00_for.on = true;
      s00_for.kap = pend.kap;
      s00_for.w = pend.w;
      s00_for.K = pend.Bq;
    }
    return AGP_OK;
  }
  bool epi_allowed() const {
    static const bool off = []() {
      const char* e = getenv("AGP_STEP_EPILOGUE");
      return e && e[0] == '0';
    }();
    if (off) return false;
    const int k = lp.kind;  // likelihoods whose local update is complete in rowstats_finish (no further kernel reads mean_f / var_f)
    return (k == AGP_LIK_GAUSSIAN && !lp.noise_dev) || k == AGP_LIK_LOGISTIC || k == AGP_LIK_STUDENTT || k == AGP_LIK_LAPLACE ||
           k == AGP_LIK_BAYESIANSVM || k == AGP_LIK_NEGBINOMIAL;
  }
  bool pro_allowed() const {
    static const bool off = []() {
      const char* e = getenv("AGP_STEP_PROLOGUE");
      return e && e[0] == '0';
    }();
    if (off || nl != 1 || mo || mo_sharded) return false;
    // only where the launch is not bound by workgroup slots: at 32 block columns (C3) the task graph already queues 1584 tile
    // workgroups through 256 slots, and the product's 27 ms of CU time inside it costs more than the kernel of its own (measured:
    // 0.70 -> 0.86-0.96 ms per step with any k-split table)
    if (mp / TILE > 16) return false;
    const int k = lp.kind;
    return k == AGP_LIK_GAUSSIAN || k == AGP_LIK_LOGISTIC || k == AGP_LIK_STUDENTT || k == AGP_LIK_LAPLACE ||
           k == AGP_LIK_BAYESIANSVM || k == AGP_LIK_NEGBINOMIAL || k == AGP_LIK_POISSON;
  }
  agp_status flush() override {
    AGPCHK(run_deferred_safe());
    s00_for.on = false;
    if (!pend.on && !pendp.on) return AGP_OK;
    Latent& g = lat[0];
    g.C_valid = false;
    if (pend.on) {
      pend.on = false;
      AGPCHK((syrk_tn<T, SY_ETA2>(ctx, pend.kap, mp, mp, pend.Bq, pend.w, 0, g.La, mp, g.eta2, pend.Kinv, mp, pend.lr, pend.r,
                                  g.eta1, pend.kinv_mu0)));
    } else {
      pendp.on = false;
      if (pendp.overlap) {  // the stand-alone step reads the whole statistic: join the collective's stream
        pendp.overlap = false;
        HIPCHK(ctx, hipStreamWaitEvent(st(), pendp.cm->ev_out, 0));
      }
      const int64_t ntri = (mp / TILE) * (mp / TILE + 1) / 2;
      hipLaunchKernelGGL((k_eta2_from_packed<T>), dim3((unsigned)(4 * ntri + (mp + 255) / 256)), dim3(256), 0, st(), stats + mp, mp,
                         g.eta2, pendp.Kinv, g.La, pendp.lr, ntri, (const T*)stats, pendp.kinv_mu0, g.eta1, mp);
    }
    LAUNCHCHK(ctx);
    g.la_state = 0;  // the epilogue left La = -2 eta2
    g.xa_valid = false;
    return AGP_OK;
  }
  agp_status step_finish() override {
    if (pro_allowed() && chol_use_dag(ctx, mp / TILE, rup64(B_last) / TILE + 1, 1) && mp / TILE <= 32) {
      Latent& g = lat[0];
      g.C_valid = false;
      pend.on = true;
      s00_for.on = false;  // (whatever was prepared belongs to an earlier pending step)
      pend.Bq = rup64(B_last);
      pend.lr = (T)cur_lr();
      pend.kap = g.kappa;
      pend.Kinv = kinv_step(g);
      pend.kinv_mu0 = kinv_mu0_step(g);
      pend.r = rbuf;
      pend.w = wbuf;
      // the bookkeeping of step_global: the posterior changes (as soon as the step is taken)
      g.la_state = 1;  // La does not hold -2 eta2: whoever wants it rebuilds it from eta2 (after flush())
      g.xa_valid = false;
      g.post_valid = false;
      g.pred_valid = g.predvar_valid = false;
      n_opt += 1;
      return kappa_released();
    }
    AGPCHK(run_deferred_safe());
    AGPCHK(step_stats(true));
    return step_global(true);
  }
  // last step
  const void* x_last = nullptr;
  // identity of the batch of the last fresh evaluation (ELBO(model, X, y), ELBO.jl:32-47) whose kappa is still in the buffers: a
  // handle that only evaluates -- the shadow handle of a SideObjective, same points every check, kernels and Z fixed -- recomputes
  // neither K_nm nor kappa = K_nm K^-1 (17 GF at 8192 x 1024) per check.  Same contract as the full-batch kappa cache: pointer
  // identity; a host that rewrites X / idx in place says so (agp_svgp_invalidate_data).  Any training step, K refresh, set_Z /
  // set_kernel clears it.
  const void* ev_x = nullptr;
  const int64_t* ev_idx = nullptr;
  int64_t ev_B = 0, ev_ldx = 0;
  bool eval_cache_ok = false;
  const void* y_last = nullptr;
  const int64_t* idx_last = nullptr;
  int64_t B_last = 0, ldx_last = 0;
  double rho_last = 1.0;

  hipStream_t st() { return ctx->stream; }
  // (round 4 measured the hyper-gradient's small launches on a side stream next to the products: 1063 -> 1077 us, every cross-stream
  //  event costs the waiting stream 7 - 12 us; removed in round 5, docs/DESIGN_LOG.md)

 protected:
  bool sparse_bufs = true;  // K_nm, kappa, the K~ partials, the kappa rows of Wbuf, stats: none in the full model (Vgp, kappa = I)
 public:
  // the descriptor's checks, before anything is allocated; a full model (Vgp, Gp) adds its own after these
  virtual agp_status check_desc() {
    m = desc.m;
    D = desc.D;
    nl = desc.n_latent;
    Bmax = desc.max_batch;
    if (m <= 0 || D <= 0 || nl <= 0 || Bmax <= 0) {
      ctx->err = "agp_svgp_create: m, D, n_latent, max_batch must be positive";
      return AGP_ERR_INVALID;
    }
    mp = rup64(m);
    Bp = rup64(Bmax);
    jitter = desc.jitter > 0 ? desc.jitter : (sizeof(T) == 8 ? 1e-4 : 1e-3);
    lp.kind = desc.lik.kind;
    lp.p0 = (T)desc.lik.p0;
    lp.p1 = (T)desc.lik.p1;
    if (lp.kind < 0 || (lp.kind > AGP_LIK_HETEROSCEDASTIC && !(lp.kind == AGP_LIK_SOFTMAX && (desc.flags & AGP_FLAG_MC)))) {
      ctx->err = "likelihood not implemented for AnalyticVI on this path";
      return AGP_ERR_UNSUPPORTED;
    }
    if (lp.kind == AGP_LIK_GAUSSIAN && !(desc.lik.p0 > 0)) return AGP_ERR_INVALID;
    if (lp.kind == AGP_LIK_GAUSSIAN && desc.lik.p1 > 0) {  // GaussianLikelihood(sigma2; opt_noise = ADAM(p1)), gaussian.jl:18-23
      lp.noise_dev = 1;
      noise_eta = desc.lik.p1;
    }
    if (lp.kind == AGP_LIK_STUDENTT && !(desc.lik.p0 > 0.5)) {
      ctx->err = "nu should be greater than 0.5";  // studentt.jl:28
      return AGP_ERR_INVALID;
    }
    if ((lp.kind == AGP_LIK_LAPLACE || lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_NEGBINOMIAL ||
         lp.kind == AGP_LIK_HETEROSCEDASTIC) && !(desc.lik.p0 > 0)) {
      ctx->err = "likelihood parameter (beta / lambda / r) must be positive";
      return AGP_ERR_INVALID;
    }
    if (lp.kind == AGP_LIK_HETEROSCEDASTIC) {  // n_latent(::HeteroscedasticGaussianLikelihood) = 2  heteroscedastic.jl:47
      if (nl != 2 || desc.latent_offset != 0) return AGP_ERR_INVALID;
    } else if (lp.kind != AGP_LIK_LOGISTICSOFTMAX && lp.kind != AGP_LIK_SOFTMAX && lp.kind != AGP_LIK_MULTIOUTPUT && nl != 1) {
      return AGP_ERR_INVALID;
    }
    if (desc.stochastic && !(desc.rm_kappa > 0.5 && desc.rm_kappa <= 1.0 && desc.rm_tau > 0)) {
      ctx->err = "RobbinsMonro: kappa in (0.5,1], tau > 0";  // optimisers.jl:7-8
      return AGP_ERR_INVALID;
    }
    return AGP_OK;
  }

  agp_status init() override {
    AGPCHK(check_desc());
    lat.resize(nl);
    const int64_t mm = mp * mp;
    for (auto& g : lat) {
      g.k.scales.assign(D, 1.0);
      AGPCHK(dmalloc(ctx, &g.scales, D + 1));  // [scale_0 .. scale_{D-1} | variance]: the kernel's device parameter array
      AGPCHK(dmalloc(ctx, &g.Z, m * D));
      AGPCHK(dmalloc(ctx, &g.L, mm));
      AGPCHK(dmalloc(ctx, &g.Xk, mm));
      AGPCHK(dmalloc(ctx, &g.Kinv, mm));
      AGPCHK(dmalloc(ctx, &g.eta1, mp));
      AGPCHK(dmalloc(ctx, &g.eta2, mm));
      AGPCHK(dmalloc(ctx, &g.La, mm));
      AGPCHK(dmalloc(ctx, &g.Xa, mm));
      AGPCHK(dmalloc(ctx, &g.v, mp));
      AGPCHK(dmalloc(ctx, &g.Sigma, mm));
      AGPCHK(dmalloc(ctx, &g.mu, mp));
      if (sparse_bufs) {  // (kappa = I: the full model has no K_nm, kappa, K~ and takes only the [eta1' ; 0] block of Wbuf)
        AGPCHK(dmalloc(ctx, &g.Knm, Bp * mp));
        AGPCHK(dmalloc(ctx, &g.kappa, Bp * mp));
        AGPCHK(dmalloc(ctx, &g.pk, (2 * mp / TILE) * Bp));
      }
      AGPCHK(dmalloc(ctx, &g.Wbuf, ((sparse_bufs ? Bp : 0) + TILE) * mp));
      AGPCHK(dmalloc(ctx, &g.DgK, mp * TILE));
      AGPCHK(dmalloc(ctx, &g.DgA, mp * TILE));
      AGPCHK(upload_scales(g));
      AGPCHK(reset_posterior(g));
    }
    ldp = Bp;
    const int ns = (int)(2 * mp / TILE);
    (void)ns;
    AGPCHK(dmalloc(ctx, &pw0, 2 * ldp > mp ? 2 * ldp : mp));
    AGPCHK(dmalloc(ctx, &pw1, 2 * ldp > mp ? 2 * ldp : mp));
    T** bv[] = {&Kt, &muf, &varf, &cbuf, &theta, &gamma, &rbuf, &wbuf, &emuf, &evarf};
    for (auto p : bv) {
      AGPCHK(dmalloc(ctx, p, nl * Bp));
      HIPCHK(ctx, hipMemsetAsync(*p, 0, sizeof(T) * nl * Bp, st()));
    }
    AGPCHK(dmalloc(ctx, &rbuf2, nl * Bp));
    AGPCHK(dmalloc(ctx, &wbuf2, nl * Bp));
    HIPCHK(ctx, hipMemsetAsync(rbuf2, 0, sizeof(T) * nl * Bp, st()));
    HIPCHK(ctx, hipMemsetAsync(wbuf2, 0, sizeof(T) * nl * Bp, st()));
    AGPCHK(dmalloc(ctx, &alpha, Bp));
    AGPCHK(dmalloc(ctx, &beta, Bp));
    AGPCHK(dmalloc(ctx, &gsum, Bp));
    AGPCHK(dmalloc(ctx, &alpha_save, Bp));
    if (sparse_bufs) AGPCHK(dmalloc(ctx, &stats, nl * stats_stride()));
    AGPCHK(dmalloc(ctx, &Tw, mm));
    AGPCHK(dmalloc(ctx, &Tw2, mm));
    AGPCHK(dmalloc(ctx, &tmpv, mp));
    AGPCHK(dmalloc(ctx, &lr_dev, 1));
    AGPCHK(dmalloc(ctx, &info_dev, 4));  // [info | infoK | flags | -]: one block, so that check_status fetches them with one copy
    infoK_dev = info_dev + 1;
    flags_dev = (int*)(info_dev + 2);
    AGPCHK(dmalloc(ctx, &scal_dev, 64));
    AGPCHK(dmalloc(ctx, &lam_dev, 1));
    AGPCHK(dmalloc(ctx, &lam_part, 2 * (Bp / 256 + 1)));
    AGPCHK(dmalloc(ctx, &noise_adam, 6));  // ADAM state [m, v, t] of the noise optimiser, + a scratch state for fresh evaluations
    HIPCHK(ctx, hipMemsetAsync(noise_adam, 0, sizeof(double) * 6, st()));
    hipLaunchKernelGGL((k_fill<T>), dim3(1), dim3(64), 0, st(), lam_dev, (int64_t)1, (T)(desc.lik.p0 > 0 ? desc.lik.p0 : 1.0));
    HIPCHK(ctx, hipMemsetAsync(info_dev, 0, sizeof(int32_t), st()));
    HIPCHK(ctx, hipMemsetAsync(infoK_dev, 0, sizeof(int32_t), st()));
    HIPCHK(ctx, hipMemsetAsync(flags_dev, 0, sizeof(int), st()));
    HIPCHK(ctx, hipMemsetAsync(info_dev + 3, 0, sizeof(int32_t), st()));  // orderK (k_logdiag_sum)
    // LogisticSoftMax state: alpha = beta = K (total classes)  logisticsoftmax.jl:43-53
    const T kk = (T)(lp.kind == AGP_LIK_LOGISTICSOFTMAX ? desc.lik.n_class : 1);
    hipLaunchKernelGGL((k_fill<T>), grid1(Bp), dim3(256), 0, st(), alpha, Bp, kk);
    hipLaunchKernelGGL((k_fill<T>), grid1(Bp), dim3(256), 0, st(), beta, Bp, kk);
    LAUNCHCHK(ctx);
    n_opt = 1;
    return AGP_OK;
  }

  ~Svgp() override {
    for (auto e : ev) dcheck(hipEventDestroy(e), __FILE_NAME__, __LINE__);
    for (auto& g : lat) {
      T* ps[] = {g.Zsc, g.zn, g.scales, g.Z, g.L, g.Xk, g.Kinv, g.mu0, g.kinv_mu0, g.eta1, g.eta2, g.La, g.Xa, g.v,
                 g.Sigma, g.mu, g.Knm, g.kappa, g.Apred, g.apred, g.Wbuf, g.DgK, g.DgA, g.pk, g.Knm_alt, g.kappa_alt, g.Wbuf_alt, g.pk_alt, g.kappa_old};
      for (T* p : ps)
        if (p) dfree(p);
    }
    if (pf_stream && sig[0]) {
      // a look-ahead still waiting for a step that was never launched must not outlive the handle
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipMemcpy(sig[0], &started_seq, sizeof(int32_t), hipMemcpyHostToDevice);
      (void)hipStreamSynchronize(pf_stream);
    }
    for (int q = 0; q < PF_SIDE; ++q) {
      if (pf_side[q]) {
        (void)hipStreamSynchronize(pf_side[q]);
        dcheck(hipStreamDestroy(pf_side[q]), __FILE_NAME__, __LINE__);
      }
      if (pf_join[q]) dcheck(hipEventDestroy(pf_join[q]), __FILE_NAME__, __LINE__);
    }
    if (pf_fork) dcheck(hipEventDestroy(pf_fork), __FILE_NAME__, __LINE__);
    if (elbo_pin) {
      dcheck(hipHostFree(elbo_pin), __FILE_NAME__, __LINE__);
      for (auto& e : elbo_ev)
        if (e) dcheck(hipEventDestroy(e), __FILE_NAME__, __LINE__);
    }
    if (pf_stream) dcheck(hipStreamDestroy(pf_stream), __FILE_NAME__, __LINE__);
    for (auto q : sig)
      if (q) dcheck(hipFree(q), __FILE_NAME__, __LINE__);
    if (arrive_dev) dcheck(hipFree(arrive_dev), __FILE_NAME__, __LINE__);
    if (pf_done) dcheck(hipEventDestroy(pf_done), __FILE_NAME__, __LINE__);
    for (auto e : step_done)
      if (e) dcheck(hipEventDestroy(e), __FILE_NAME__, __LINE__);
    T* ps[] = {rbuf2, wbuf2, pw0, pw1, Kt, muf, varf, cbuf, theta, gamma, rbuf, wbuf, alpha, beta, gsum, alpha_save, emuf,
               evarf, stats, Tw, Tw2, tmpv, lr_dev, Kstar, ppm, ppv, pmu, pvar, s00buf, pg_W, pg_gm, pg_gv};
    for (T* p : ps)
      if (p) dfree(p);
    T* hps[] = {hyH1, hyH2, hyH3, hy_gmu, hy_gs, hy_muf, hy_pZ, hy_dZ, hyKap, hyKnm, hy_upart, hy_pZ2};
    for (T* p : hps)
      if (p) dfree(p);
    double* hds[] = {hy_pvar, hy_pscale, hy_g, hy_tied, hy_pvar2, hy_pscale2};
    for (double* p : hds)
      if (p) dfree(p);
    for (auto& g : lat) {
      free_online(g);
      T* sp[] = {g.sKinv, g.sXk, g.skinv_mu0, g.Cmat};
      for (T* q : sp)
        if (q) dfree(q);
      if (g.kadam) dfree(g.kadam);
      if (g.z_am) dfree(g.z_am);
      if (g.z_av) dfree(g.z_av);
    }
    T* mops[] = {A_dev, mo_mixm, mo_mixv, mo_th, mo_cc, mo_th_save, mo_pmu, mo_pvar, fall};
    for (T* p : mops)
      if (p) dfree(p);
    double* dps[] = {gradA_dev, am_dev, av_dev};
    for (double* p : dps)
      if (p) dfree(p);
    if (pg_part) dfree(pg_part);
    if (info_dev) dfree(info_dev);  // (infoK_dev, flags_dev point into the same block)
    if (scal_dev) dfree(scal_dev);
    if (gh_dev) dfree(gh_dev);
    if (lam_dev) dfree(lam_dev);
    if (lam_part) dfree(lam_part);
    if (noise_adam) dfree(noise_adam);
    if (frob_part) dfree(frob_part);
    if (es_mu) dfree(es_mu);
    if (es_var) dfree(es_var);
    if (es_part) dfree(es_part);
    if (es_scal) dfree(es_scal);
    if (logdetK_dev) dfree(logdetK_dev);
  }

  // host copy of the kernel parameters -> device array [scales | variance] (set_kernel; the training loop never comes here: the
  // hyper step's ADAM runs on the device, k_adam_kernel_params)
  agp_status upload_scales(Latent& g) {
    std::vector<T> h(D + 1);
    for (int64_t d = 0; d < D; ++d) h[d] = (T)g.k.scales[d];
    h[D] = (T)g.k.variance;
    HIPCHK(ctx, hipMemcpyAsync(g.scales, h.data(), sizeof(T) * (D + 1), hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));  // h goes out of scope
    g.host_params_stale = false;
    return AGP_OK;
  }
  // device -> host copy, only where host logic needs the values (get_kernel, prediction set-up, the online model's hand-over):
  // synchronises
  agp_status params_to_host(Latent& g) {
    if (!g.host_params_stale) return AGP_OK;
    std::vector<T> h(D + 1);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), g.scales, sizeof(T) * (D + 1), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    for (int64_t d = 0; d < D; ++d) g.k.scales[d] = (double)h[d];
    g.k.variance = (double)h[D];
    g.host_params_stale = false;
    return AGP_OK;
  }
  // the variance argument of the kernels that take (scales, variance): the host value, or -1 = "read element D of the device
  // parameter array" while the host copy is stale (between a device-side ADAM step and the next params_to_host)
  T kvar(const Latent& g) const { return g.host_params_stale ? T(-1) : (T)g.k.variance; }

  // VarPosterior{T}(dim): mu = 0, Sigma = I, eta1 = 0, eta2 = -I/2   (posterior.jl:29-37)
  agp_status reset_posterior(Latent& g) {
    HIPCHK(ctx, hipMemsetAsync(g.eta1, 0, sizeof(T) * mp, st()));
    HIPCHK(ctx, hipMemsetAsync(g.v, 0, sizeof(T) * mp, st()));
    hipLaunchKernelGGL((k_set_identity<T>), grid2(mp, mp), blk2, 0, st(), g.eta2, mp, mp, T(-0.5));
    hipLaunchKernelGGL((k_set_identity<T>), grid2(mp, mp), blk2, 0, st(), g.La, mp, mp, T(1));
    hipLaunchKernelGGL((k_set_identity<T>), grid2(mp, mp), blk2, 0, st(), g.Xa, mp, mp, T(1));
    LAUNCHCHK(ctx);
    g.post_valid = false;
    g.pred_valid = g.predvar_valid = false;
    g.la_state = 0;
    g.xa_valid = false;
    return AGP_OK;
  }

  agp_status set_kernel(int l, const agp_kernel_desc* k) override {
    if (l < 0 || l >= nl || !k) return AGP_ERR_INVALID;
    if (k->kind < 0 || k->kind > AGP_K_EXPONENTIAL || !(k->variance > 0)) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    g.k.kind = k->kind;
    g.k.variance = k->variance;
    g.k.ard = k->ard != 0;
    g.k.has_variance = k->has_variance != 0;
    g.k.has_transform = k->has_transform != 0 || k->ard != 0;
    for (int64_t d = 0; d < D; ++d) g.k.scales[d] = k->ard ? k->ard_scales_host[d] : k->scale;
    g.K_stale = true;
    g.kappa_valid = g.kappa_eval = false;
    g.zsc_valid = false;
    pf_valid = false;
    g.pred_valid = g.predvar_valid = false;
    return upload_scales(g);
  }

  agp_status set_Z(int l, const void* z, int64_t ldz) override {
    if (l < 0 || l >= nl || !z || ldz < D) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    HIPCHK(ctx, hipMemcpy2DAsync(g.Z, sizeof(T) * D, z, sizeof(T) * ldz, sizeof(T) * D, m, hipMemcpyDeviceToDevice,
                                 st()));
    g.K_stale = true;
    g.kappa_valid = g.kappa_eval = false;
    g.zsc_valid = false;
    pf_valid = false;
    g.pred_valid = g.predvar_valid = false;
    return AGP_OK;
  }

  agp_status get_Z(int l, void* z, int64_t ldz) override {
    if (l < 0 || l >= nl || !z || ldz < D) return AGP_ERR_INVALID;
    HIPCHK(ctx, hipMemcpy2DAsync(z, sizeof(T) * ldz, lat[l].Z, sizeof(T) * D, sizeof(T) * D, m,
                                 hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }

  agp_status set_mu0(int l, const void* mu0) override {
    if (l < 0 || l >= nl) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    if (!mu0) {
      if (g.mu0) (void)hipFree(g.mu0);
      if (g.kinv_mu0) (void)hipFree(g.kinv_mu0);
      g.mu0 = g.kinv_mu0 = nullptr;
      return AGP_OK;
    }
    if (!g.mu0) {
      AGPCHK(dmalloc(ctx, &g.mu0, mp));
      AGPCHK(dmalloc(ctx, &g.kinv_mu0, mp));
    }
    HIPCHK(ctx, hipMemsetAsync(g.mu0, 0, sizeof(T) * mp, st()));
    HIPCHK(ctx, hipMemcpyAsync(g.mu0, mu0, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    g.K_stale = true;  // K^-1 mu0 must be refreshed
    return AGP_OK;
  }

  // compute_K : cholesky(kernelmatrix(k, Z) + jitt*I) ; inv(K)      latentgp.jl:205-207, analyticVI.jl:179
  agp_status refresh_K() override {
    bool any = false;
    if (pend.on)  // the pending natural-gradient step belongs to the kernel matrices it was computed with
      for (auto& g : lat)
        if (g.K_stale) {
          AGPCHK(flush());
          break;
        }
    for (auto& g : lat) {
      if (!g.K_stale) continue;
      any = true;
      // the factorisations of K_ZZ latch their failures in a word of their own (infoK_dev): what an earlier asynchronous step
      // latched (K~ <= 0, a non-SPD -2*eta2) stays in info_dev / flags_dev and is reported as what it is by check_status
      {
        AGPCHK(ensure_zsc(g));
        (void)launch_kernelmatrix<T>(ctx, st(), (const T*)g.Z, D, (const int64_t*)nullptr, m, (const T*)g.Z, D, m, D,
                                     (const T*)g.scales, g.k.kind, kvar(g), g.L, mp, mp, mp, 1, (T)jitter,
                                     (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
        LAUNCHCHK(ctx);
        // the task graph's in-stream fallback recomputes K from the inducing points (the factor overwrote it) and forms L^-1 itself
        SafeSrc<T> src{};
        src.want_x = 1;
        src.kz = g.Z;
        src.ldz = D;
        src.mz = m;
        src.Dz = D;
        src.kscales = g.scales;
        src.kkind = g.k.kind;
        src.kvariance = kvar(g);
        src.kjitter = (T)jitter;
        if (!logdetK_dev) AGPCHK(dmalloc(ctx, &logdetK_dev, nl));
        const int li = (int)(&g - lat.data());
        PotrfReq<T> rq{};
        rq.A = g.L, rq.ld = mp, rq.n = mp, rq.X = g.Xk, rq.ldx = mp, rq.Dg = g.DgK, rq.do_x = 1, rq.info_dev = infoK_dev, rq.nvalid = m;
        rq.safe = &src;
        // K^-1 = X' X (and log det K) by product workgroups of the same launch (task graph, rq.p_done), else below
        rq.Pout = g.Kinv, rq.ld_out = logdetK_dev + li, rq.ld_status = info_dev;
        AGPCHK(potrf_fused<T>(ctx, rq));
        bool ld_done = rq.p_done;
        if (!rq.p_done)
          AGPCHK(xtx_padded<T>(ctx, g.Xk, mp, mp, g.Kinv, mp, (const T*)g.DgK, m, logdetK_dev + li, info_dev, &ld_done));
        if (!ld_done)
          hipLaunchKernelGGL((k_logdiag_sum<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.DgK, m, logdetK_dev + li, info_dev);
        LAUNCHCHK(ctx);
        g.logdet_pending = true;
        if (!refresh_lazy) {
          // log det K and the status, read now: one synchronisation per refreshed latent.  (refresh_lazy: a refresh issued from
          // inside the training loop -- the hyper step moved the kernel -- leaves both on the device: log det K is fetched when an
          // ELBO asks for it, a non-SPD K_ZZ stays latched in infoK_dev and is reported by agp_svgp_check_status)
          int32_t info = 0;
          HIPCHK(ctx, hipMemcpyAsync(&info, infoK_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st()));
          AGPCHK(resolve_logdet(g));  // synchronises
          if (info != 0) {
            HIPCHK(ctx, hipMemsetAsync(infoK_dev, 0, sizeof(int32_t), st()));
            for (auto& q : lat) q.K_stale = true;
            // a failure an earlier asynchronous step latched (K~ <= 0 makes everything after it NaN, kernel parameters included)
            // is the root cause and is what the reference would have thrown first
            AGPCHK(check_status());
            ctx->err = info < 0 ? std::string("task-graph factorisation of K_ZZ aborted: a tile dependency never arrived")
                                : "PosDefException: K_ZZ + jitter*I is not positive definite; leading minor " + std::to_string(info);
            return info < 0 ? AGP_ERR_HIP : AGP_ERR_NOT_POSDEF;
          }
        }
      }
      if (g.mu0) {
        hipLaunchKernelGGL((k_symv<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Kinv, mp, mp, (const T*)g.mu0,
                           g.kinv_mu0);
        LAUNCHCHK(ctx);
      }
      g.K_stale = false;
      g.C_valid = false;  // (C = kappa' diag(w) kappa + K^-1 / 4 of a step under the kernel matrices before this refresh)
      if (tw2_kis_of == (int)(&g - lat.data())) tw2_kis_of = -1;
      // (under AGP_FLAG_STALE_K a full-batch run keeps the step's kernel matrices across the refresh of the fresh set)
      g.kappa_eval = false;
      if (!(g.stale_on && !desc.stochastic)) g.kappa_valid = false;
      g.pred_valid = g.predvar_valid = false;
    }
    for (auto& g : lat)
      if (g.on && (g.on_dirty || any)) AGPCHK(online_refresh(g));
    return AGP_OK;
  }

  // ---- OnlineSVGP streaming prior ------------------------------------------------------------------------------------
  void free_online(Latent& g) {
    T* ps[] = {g.Za, g.invDa, g.peta1, g.kappa_a, g.Kab, g.Kta, g.onT, g.onQ, g.kinv_mu0_on, g.Kinv_on, g.ov0, g.ov1,
               g.oh1, g.oh2, g.oh3};
    for (T* p : ps)
      if (p) dfree(p);
    g.Za = g.invDa = g.peta1 = g.kappa_a = g.Kab = g.Kta = g.onT = g.onQ = g.kinv_mu0_on = g.Kinv_on = g.ov0 = g.ov1 = nullptr;
    g.oh1 = g.oh2 = g.oh3 = nullptr;
    g.on = false;
  }

  agp_status set_online_prior(int l, const void* za, int64_t ldza, int64_t ma, const void* invDa, int64_t ldi,
                              const void* peta1, double prevLa) override {
    if (l < 0 || l >= nl || ma <= 0 || !invDa || !peta1 || ldi < ma || (za && ldza < D)) return AGP_ERR_INVALID;
    if (desc.stochastic) {  // set_rho!(model, ...) in the stochastic branch of onlinetraining.jl:52 references an undefined name
      ctx->err = "OnlineSVGP runs with AnalyticVI() (full batches); the reference's stochastic branch is broken";
      return AGP_ERR_UNSUPPORTED;
    }
    if (!za && ma != m) return AGP_ERR_INVALID;  // first batch: kappa_a = I needs the sizes to agree
    Latent& g = lat[l];
    free_online(g);
    g.ma = ma;
    g.map = rup64(ma);
    const int64_t map = g.map;
    AGPCHK(dmalloc(ctx, &g.invDa, map * map));
    AGPCHK(dmalloc(ctx, &g.peta1, map));
    AGPCHK(dmalloc(ctx, &g.kappa_a, map * mp));
    AGPCHK(dmalloc(ctx, &g.Kab, map * mp));
    AGPCHK(dmalloc(ctx, &g.Kta, map * map));
    AGPCHK(dmalloc(ctx, &g.onT, map * mp));
    AGPCHK(dmalloc(ctx, &g.onQ, std::max(map * map, mp * mp)));
    AGPCHK(dmalloc(ctx, &g.kinv_mu0_on, mp));
    AGPCHK(dmalloc(ctx, &g.Kinv_on, mp * mp));
    AGPCHK(dmalloc(ctx, &g.ov0, map));
    AGPCHK(dmalloc(ctx, &g.ov1, map));
    AGPCHK(dmalloc(ctx, &g.oh1, map * mp));
    AGPCHK(dmalloc(ctx, &g.oh2, map * mp));
    AGPCHK(dmalloc(ctx, &g.oh3, map * mp));
    hipLaunchKernelGGL((k_copy2d_zero<T>), grid2(map, map), blk2, 0, st(), (const T*)invDa, ldi, ma, ma, g.invDa, map, map, map);
    HIPCHK(ctx, hipMemsetAsync(g.peta1, 0, sizeof(T) * map, st()));
    HIPCHK(ctx, hipMemcpyAsync(g.peta1, peta1, sizeof(T) * ma, hipMemcpyDeviceToDevice, st()));
    if (za) {
      AGPCHK(dmalloc(ctx, &g.Za, ma * D));
      HIPCHK(ctx, hipMemcpy2DAsync(g.Za, sizeof(T) * D, za, sizeof(T) * ldza, sizeof(T) * D, ma, hipMemcpyDeviceToDevice, st()));
    }
    LAUNCHCHK(ctx);
    g.on_first = za == nullptr;
    g.prevLa = prevLa;
    g.on = true;
    g.on_dirty = true;
    return AGP_OK;
  }

  agp_status online_refresh(Latent& g) {
    const int64_t map = g.map, ma = g.ma;
    if (g.on_first) {  // compute_kappa with empty Z_a (latentgp.jl:220-223): K_ab = 0, kappa_a = I, K~_a = 0
      HIPCHK(ctx, hipMemsetAsync(g.Kab, 0, sizeof(T) * map * mp, st()));
      HIPCHK(ctx, hipMemsetAsync(g.kappa_a, 0, sizeof(T) * map * mp, st()));
      HIPCHK(ctx, hipMemsetAsync(g.Kta, 0, sizeof(T) * map * map, st()));
      hipLaunchKernelGGL((k_add_diag<T>), grid1(ma), dim3(256), 0, st(), g.kappa_a, mp, ma, T(1));
    } else {
      dim3 gk((unsigned)(mp / TILE), (unsigned)(map / TILE));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)g.Za, D, (const int64_t*)nullptr, ma,
                         (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), g.Kab, mp, map, mp, 0, T(0),
                         (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Kab, mp, g.Kinv, mp, map, mp, mp, 0, g.kappa_a, mp, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));
      dim3 ga((unsigned)(map / TILE), (unsigned)(map / TILE));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)g.Za, D, (const int64_t*)nullptr, ma,
                         (const T*)g.Za, D, ma, D, (const T*)g.scales, g.k.kind, kvar(g), g.Kta, map, map, map, 0,
                         T(0), (const T*)nullptr, (T*)nullptr, (int64_t)0);
      hipLaunchKernelGGL((k_add_diag<T>), grid1(ma), dim3(256), 0, st(), g.Kta, map, ma, (T)jitter);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.kappa_a, mp, g.Kab, mp, map, map, mp, 0, g.onQ, map, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));
      hipLaunchKernelGGL((k_sub2d<T>), grid2(ma, ma), blk2, 0, st(), g.Kta, (const T*)g.onQ, map, ma);
    }
    LAUNCHCHK(ctx);
    // eta1 target gains kappa_a' eta1_a ; -eta2 target gains kappa_a' invD_a kappa_a / 2  (analyticVI.jl:197-201): folded into
    // the K^-1 mu0 and K^-1 operands of the step kernels
    hipLaunchKernelGGL((k_gemv_cols<T>), grid1(mp), dim3(256), 0, st(), (const T*)g.kappa_a, mp, ma, mp, (const T*)g.peta1,
                       g.kinv_mu0_on);
    hipLaunchKernelGGL((k_axpby<T>), grid1(mp), dim3(256), 0, st(), mp, T(1), (const T*)g.kinv_mu0_on, T(1),
                       (const T*)g.kinv_mu0, g.kinv_mu0_on);
    {
      dim3 g1((unsigned)(mp / TILE), (unsigned)(map / TILE));  // T = invD_a kappa_a  (invD_a symmetric)
      hipLaunchKernelGGL((k_gemm_tn<T, 1>), g1, dim3(NTHREADS), 0, st(), (const T*)g.invDa, map, (const T*)g.kappa_a, mp, map,
                         g.onT, mp);
      dim3 g2((unsigned)(mp / TILE), (unsigned)(mp / TILE));   // kappa_a' T
      hipLaunchKernelGGL((k_gemm_tn<T, 1>), g2, dim3(NTHREADS), 0, st(), (const T*)g.kappa_a, mp, (const T*)g.onT, mp, map,
                         g.onQ, mp);
    }
    HIPCHK(ctx, hipMemcpyAsync(g.Kinv_on, g.Kinv, sizeof(T) * mp * mp, hipMemcpyDeviceToDevice, st()));
    hipLaunchKernelGGL((k_add_sym<T>), grid2(m, m), blk2, 0, st(), (const T*)g.Kinv, (const T*)g.onQ, mp, m, g.Kinv_on);
    LAUNCHCHK(ctx);
    g.on_dirty = false;
    return AGP_OK;
  }

  // (invD_a, eta1_a, L_a) of save_old_gp! (onlinetraining.jl:170-180) from the current posterior
  agp_status online_snapshot(int l, void* invDa_out, int64_t ldi, void* eta1_out, double* prevLa_host) override {
    if (l < 0 || l >= nl || !invDa_out || !eta1_out || !prevLa_host || ldi < m) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    AGPCHK(refresh_K());
    AGPCHK(materialize(g));
    hipLaunchKernelGGL((k_axpby<T>), grid1(mp * mp), dim3(256), 0, st(), mp * mp, T(-2), (const T*)g.eta2, T(-1),
                       (const T*)g.Kinv, Tw);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpy2DAsync(invDa_out, sizeof(T) * ldi, Tw, sizeof(T) * mp, sizeof(T) * m, m, hipMemcpyDeviceToDevice,
                                 st()));
    HIPCHK(ctx, hipMemcpyAsync(eta1_out, g.eta1, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    hipLaunchKernelGGL((k_logdiag_sum<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.DgA, m, scal_dev + 2);
    hipLaunchKernelGGL((k_dot<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.mu, (const T*)g.eta1, m, scal_dev + 3);
    LAUNCHCHK(ctx);
    double h[2];
    HIPCHK(ctx, hipMemcpyAsync(h, scal_dev + 2, sizeof(double) * 2, hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    // (-logdet Sigma + logdet K - mu'eta1)/2 with logdet Sigma = -2 sum log diag chol(-2 eta2)
    AGPCHK(resolve_logdet(g));
    *prevLa_host = 0.5 * (2.0 * h[0] + 2.0 * g.half_logdetK - h[1]);
    return AGP_OK;
  }

  // local variables and expectation gradients of `src` (same likelihood, same batch capacity) become this handle's:
  // first iteration of a new streaming batch (onlinetraining.jl:78-104: local update under the OLD inducing points)
  agp_status adopt_local(SvgpBase* srcb) override {
    Svgp<T>* src = dynamic_cast<Svgp<T>*>(srcb);
    if (!src || src == this || src->nl != nl || src->Bp != Bp || src->lp.kind != lp.kind ||
        src->ctx->device != ctx->device || src->ctx->stream != ctx->stream)
      return AGP_ERR_INVALID;  // both handles must enqueue on the same stream: the copies are ordered by it
    AGPCHK(src->lsm_finish());
    const size_t nb = sizeof(T) * nl * Bp;
    T* d[] = {cbuf, theta, gamma, rbuf, wbuf};
    T* s0[] = {src->cbuf, src->theta, src->gamma, src->rbuf, src->wbuf};
    for (int i = 0; i < 5; ++i) HIPCHK(ctx, hipMemcpyAsync(d[i], s0[i], nb, hipMemcpyDeviceToDevice, st()));
    HIPCHK(ctx, hipMemcpyAsync(alpha, src->alpha, sizeof(T) * Bp, hipMemcpyDeviceToDevice, st()));
    HIPCHK(ctx, hipMemcpyAsync(lam_dev, src->lam_dev, sizeof(T), hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }

  // extraKL (KLdivergences.jl:30-54)
  agp_status extra_kl(Latent& g, double* out) {
    const int64_t map = g.map, ma = g.ma;
    AGPCHK(materialize(g));
    hipLaunchKernelGGL((k_gemv_rows<T>), grid1(ma * 64), dim3(256), 0, st(), (const T*)g.kappa_a, mp, ma, mp, (const T*)g.mu,
                       g.ov0);                                                     // kappa_a mu
    AGPCHK(frob_dot((const T*)g.invDa, (const T*)g.Kta, map, ma,
                    scal_dev + 48));  // tr(invD_a K~_a)
    LAUNCHCHK(ctx);
    AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.kappa_a, mp, g.Sigma, mp, map, mp, mp, 0, g.onT, mp, nullptr, 0, nullptr, nullptr,
                                  nullptr, 0)));                                 // kappa_a Sigma
    AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.onT, mp, g.kappa_a, mp, map, map, mp, 0, g.onQ, map, nullptr, 0, nullptr, nullptr,
                                  nullptr, 0)));                                 // (kappa_a Sigma) kappa_a'
    AGPCHK(frob_dot((const T*)g.invDa, (const T*)g.onQ, map, ma, scal_dev + 49));
    hipLaunchKernelGGL((k_dot<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.peta1, (const T*)g.ov0, ma, scal_dev + 50);
    hipLaunchKernelGGL((k_symv<T>), grid1(ma * 64), dim3(256), 0, st(), (const T*)g.invDa, map, ma, (const T*)g.ov0, g.ov1);
    hipLaunchKernelGGL((k_dot<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.ov0, (const T*)g.ov1, ma, scal_dev + 51);
    LAUNCHCHK(ctx);
    double h[4];
    HIPCHK(ctx, hipMemcpyAsync(h, scal_dev + 48, sizeof(double) * 4, hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    *out = g.prevLa - 0.5 * (h[0] + h[1]) + h[2] - 0.5 * h[3];
    return AGP_OK;
  }

  // the ready-made Y tiles of every kernel matrix against this latent's inducing points (k_kernelmatrix_mma)
  agp_status ensure_zsc(Latent& g) {
    if (g.zsc_valid || !kmm_usable(D)) return AGP_OK;
    const int Dp = kmm_dp(D);
    if (!g.Zsc) {
      AGPCHK(dmalloc(ctx, &g.Zsc, mp * Dp));
      AGPCHK(dmalloc(ctx, &g.zn, mp));
    }
    hipLaunchKernelGGL((k_scale_rows<T>), dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, st(), (const T*)g.Z, D, m, mp, D, Dp,
                       (const T*)g.scales, g.Zsc, g.zn);
    LAUNCHCHK(ctx);
    g.zsc_valid = true;
    return AGP_OK;
  }

  // which K-derived matrices the STEP uses (online prior folded in > frozen copies of AGP_FLAG_STALE_K > the fresh ones)
  const T* kinv_kappa(const Latent& g) const { return g.stale_on ? g.sKinv : g.Kinv; }
  const T* kinv_step(const Latent& g) const { return g.on ? g.Kinv_on : (g.stale_on ? g.sKinv : g.Kinv); }
  const T* kinv_mu0_step(const Latent& g) const { return g.on ? g.kinv_mu0_on : (g.stale_on ? g.skinv_mu0 : g.kinv_mu0); }
  bool stale_mode() const { return (desc.flags & AGP_FLAG_STALE_K) != 0; }

  // compute_K where train! starts and ends (training.jl:41-43,107): with AGP_FLAG_STALE_K this is the only thing that ends
  // the staleness; without the flag it is plain refresh_K
  agp_status refresh_K_explicit() override {
    for (auto& g : lat) g.stale_on = false;
    return refresh_K();
  }

  agp_status check_batch(int64_t B) {
    if (B <= 0 || B > Bmax) {  // training.jl:27-29
      ctx->err = "The size of mini-batch " + std::to_string(B) + " is incorrect (negative or bigger than max_batch)";
      return AGP_ERR_BAD_BATCH;
    }
    return AGP_OK;
  }

  // the likelihood updates that need more than one point (lambda of Poisson / Heteroscedastic, the optimised Gaussian noise): after the
  // point-wise part, on mean_f / var_f of the batch
  agp_status lik_tail(const void* y, const int64_t* idx, int64_t B, double rho, bool fresh) {
    if (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev) {  // sigma2 step, then theta / gradients with the new sigma2  gaussian.jl:56-72
      const int nb = (int)((B + 255) / 256);
      // a fresh evaluation (external ELBO: new local variables, ELBO.jl:32-47) steps sigma2 from a NEW optimiser state and throws
      // that state away, as the reference does; the training state is left alone
      double* ad = fresh ? noise_adam + 3 : noise_adam;
      if (fresh) HIPCHK(ctx, hipMemsetAsync(ad, 0, sizeof(double) * 3, st()));
      hipLaunchKernelGGL((k_noise_partial<T>), dim3(nb), dim3(256), 0, st(), B, (const T*)y, idx, (const T*)muf, (const T*)varf,
                         lam_part);
      if (lam_deferred) {
        hipLaunchKernelGGL(k_lambda_reduce, dim3(1), dim3(256), 0, st(), nb, 1, (const double*)lam_part, (double)B, scal_dev + 60);
      } else {
        hipLaunchKernelGGL((k_noise_finish<T>), dim3(1), dim3(256), 0, st(), nb, (const double*)lam_part, (double)B,
                           (const double*)nullptr, noise_eta, 0.9, 0.999, 1e-8, ad, lam_dev);
        hipLaunchKernelGGL((k_gauss_grads<T>), dim3(nb), dim3(256), 0, st(), B, (T)rho, (const T*)y, idx, (const T*)lam_dev, theta,
                           cbuf, rbuf, wbuf);
      }
      LAUNCHCHK(ctx);
    } else if (lp.kind == AGP_LIK_POISSON) {  // lambda <- sum(y) / sum E[logistic(f)]   poisson.jl:78
      if (gh_n <= 0) {
        ctx->err = "PoissonLikelihood: install the Gauss-Hermite rule first (agp_svgp_set_quadrature)";
        return AGP_ERR_INVALID;
      }
      const int nb = (int)((B + 255) / 256);
      hipLaunchKernelGGL((k_poisson_partial<T>), dim3(nb), dim3(256), 0, st(), B, (const T*)y, idx, (const T*)muf,
                         (const T*)varf, gh_n, (const double*)gh_dev, (const double*)(gh_dev + gh_n), lam_part);
      if (lam_deferred)  // batch-sharded: the sums travel first (cavi_step_multi), lambda_finish_reduced() follows
        hipLaunchKernelGGL(k_lambda_reduce, dim3(1), dim3(256), 0, st(), nb, 2, (const double*)lam_part, (double)B, scal_dev + 60);
      else
        hipLaunchKernelGGL((k_lambda_finish<T>), dim3(1), dim3(256), 0, st(), nb, 2, (const double*)lam_part, 0, (double)B,
                           lam_dev);
      LAUNCHCHK(ctx);
    } else if (lp.kind == AGP_LIK_HETEROSCEDASTIC) {  // heteroscedastic.jl:71-129
      const int nb = (int)((B + 255) / 256);
      hipLaunchKernelGGL((k_hetero_local<T>), dim3(nb), dim3(256), 0, st(), B, Bp, (const T*)y, idx, (const T*)muf,
                         (const T*)varf, (const T*)lam_dev, cbuf, gamma, theta, lam_part);
      if (lam_deferred) {
        hipLaunchKernelGGL(k_lambda_reduce, dim3(1), dim3(256), 0, st(), nb, 1, (const double*)lam_part, (double)B, scal_dev + 60);
      } else {
        hipLaunchKernelGGL((k_lambda_finish<T>), dim3(1), dim3(256), 0, st(), nb, 1, (const double*)lam_part, 1, (double)B,
                           lam_dev);
        hipLaunchKernelGGL((k_hetero_grads<T>), dim3(nb), dim3(256), 0, st(), B, Bp, (T)rho, (const T*)y, idx,
                           (const T*)lam_dev, (const T*)gamma, theta, rbuf, wbuf);
      }
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }

  // compute_kappa + mean_f/var_f + local update
  agp_status step_local(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho,
                        bool fresh) override {
    AGPCHK(check_batch(B));
    if (!x || !y || ldx < D) return AGP_ERR_INVALID;
    lsm_finished = false;
    for (auto& g : lat) g.C_valid = false;  // the local variables (theta, w) and kappa it belongs to are about to change
    dag_tick(ctx);
    refresh_lazy = !fresh;  // a refresh issued from inside the training loop (the hyper step moved the kernel) does not synchronise
    const agp_status rks = refresh_K();
    refresh_lazy = false;
    AGPCHK(rks);
    const int64_t Bq = rup64(B);
    const int ns = (int)(2 * mp / TILE);
    const bool reuse = !desc.stochastic && !fresh && x == x_last && idx == idx_last && B == B_last && ldx == ldx_last;
    const bool reuse_eval = fresh && eval_cache_ok && x == ev_x && idx == ev_idx && B == ev_B && ldx == ev_ldx;
    if (!fresh)
      for (auto& g : lat) g.kappa_eval = false;  // (a training step takes the buffers)
    const bool prefetched = pf_valid && !fresh && x == pf_x && idx == pf_idx && B == pf_B && ldx == pf_ldx;
    // how many problems one task-graph launch may take (0: none fits, plain launches)
    int dag_nb = 0;
    for (int q = DAG_MAX_NB; q >= 1 && !dag_nb; --q)
      if (chol_use_dag(ctx, mp / TILE, Bq / TILE + 1, q)) dag_nb = q;
    // single latent on the task graph: the launch itself tells the look-ahead stream that the step
    // before has released its kappa buffers (DagSync) -- no event record on this stream
    // a pending natural-gradient step rides on this step's task-graph launch when this is the steady state of a training loop
    // (kappa of the minibatch already there -- look-ahead or kept --, one latent on the task graph); otherwise it is taken now
    const bool take_pend = (pend.on || pendp.on) && !fresh && nl == 1 && dag_nb > 0 &&
                           (prefetched || (reuse && lat[0].kappa_valid)) && pro_allowed() && mp / TILE <= 32 &&
                           (pendp.on || pend.Bq >= TILE);
    // ... with the row statistics as its epilogue: then the previous step's deferred launch, whichever call below enqueues it, also
    // prepares the head of this one (ProArgs::pre) -- in every protocol alike, so that the trajectory does not depend on which
    const bool pre_want = take_pend && in_cavi_step && epi_allowed();
    StepSync ssync{};
    const bool sync_step = sig_state == 1 && !fresh && nl == 1 && dag_nb > 0 &&
                           !(lat[0].la_state == 1 && lat[0].xa_valid);
    if (sync_step) {
      ssync.ds.started = sig[0];
      ssync.ds.seq = started_seq + 1;
    } else if (rel_pending) {
      // the release of the previous step's kappa buffers becomes an event here, before anything of this step is enqueued (the
      // look-ahead waiting for it is meant to run next to this step's factorisation).  The previous step's deferred fallback goes
      // first: if it really re-runs it rewrites that step's Wbuf and reads its pk -- the buffers this event releases
      AGPCHK(run_deferred_safe(nullptr, 0, pre_want));
      slot_kind[rel_slot] = 0;
      HIPCHK(ctx, hipEventRecord(step_done[rel_slot], st()));
      rel_pending = false;
    }
    bool use_pro = false;
    if (pend.on || pendp.on) {
      use_pro = take_pend;
      if (!use_pro) AGPCHK(flush());
    }
    // the row statistics of this step as the epilogue of its task-graph launch, the launch's fallback deferred to the next step
    const bool use_epi = pre_want;
    if (prefetched) {  // kappa of this minibatch was produced on the prefetch stream: adopt those buffers
      if (sig_state == 1) {  // (the look-ahead's completion word is polled in-stream; without signal memory: an event wait)
        if (sdef.on) {  // the previous step's deferred fallback launch carries this step's wait for its look-ahead
          AGPCHK(run_deferred_safe((const int32_t*)sig[1], pf_seq, use_epi));
        } else {
          hipLaunchKernelGGL(k_wait_ge_fast, dim3(1), dim3(64), 0, st(), (const int32_t*)sig[1], pf_seq, info_dev);
          LAUNCHCHK(ctx);
        }
      } else {
        AGPCHK(run_deferred_safe(nullptr, 0, use_epi));
        HIPCHK(ctx, hipStreamWaitEvent(st(), pf_done, 0));
      }
      for (auto& g : lat) {
        std::swap(g.Knm, g.Knm_alt);
        std::swap(g.Wbuf, g.Wbuf_alt);
        std::swap(g.pk, g.pk_alt);
        // kappa rotates through three buffers: the one just left may still be read by this step's prologue (pending step), so
        // the next look-ahead target is the one before it
        T* left = g.kappa;
        g.kappa = g.kappa_alt;
        g.kappa_alt = g.kappa_old;
        g.kappa_old = left;
      }
      pf_valid = false;
    }
    AGPCHK(run_deferred_safe(nullptr, 0, use_epi));  // (full-batch steps: no look-ahead to wait for)
    CholBatch<T> merged_bt{};  // single latent on the task graph: fallback + row statistics share a launch (k_safe_rowstats)
    SafeSrc<T> merged_src{};
    bool merged_safe = false;
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      const bool keep = (reuse && g.kappa_valid) || (reuse_eval && g.kappa_eval);
      g.keep_last = keep;
      if (prefetched) {
        // nothing to compute
      } else if (!keep) {
        AGPCHK(ensure_zsc(g));
        dim3 gk((unsigned)(mp / TILE), (unsigned)(Bq / TILE));
        (void)launch_kernelmatrix<T>(ctx, st(), (const T*)x, ldx, idx, B, (const T*)g.Z,
                           D, m, D, (const T*)g.scales, g.k.kind, kvar(g), g.Knm, mp, Bq, mp, 0, T(0),
                           (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
        LAUNCHCHK(ctx);
        AGPCHK((gemm_nt<T, EPI_KAPPA>(ctx, g.Knm, mp, kinv_kappa(g), mp, Bq, mp, mp, 0, g.kappa, mp, g.Knm, mp, nullptr,
                                      g.pk, g.Wbuf, ldp)));
        g.kappa_valid = !desc.stochastic && !fresh;
        g.kappa_eval = fresh && eval_cache_ok;
      } else if (!(g.la_state == 1 && g.xa_valid)) {  // (W = kappa Xa' below writes Wbuf itself)
        HIPCHK(ctx, hipMemcpyAsync(g.Wbuf, g.kappa, sizeof(T) * Bq * mp, hipMemcpyDeviceToDevice, st()));
      }
      // When the factor of the CURRENT -2*eta2 and its inverse X_a are still around (a materialize() since the last
      // global update: ELBO callback, hyper-parameter step, prediction), W = kappa X_a' and v = X_a eta1 are one GEMM and
      // one triangular mat-vec -- no second 16-launch factorisation chain of the same matrix.
      g.via_inverse = g.la_state == 1 && g.xa_valid;
      if (g.via_inverse) {
        AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.kappa, mp, g.Xa, mp, Bq, mp, mp, 1, g.Wbuf, mp, nullptr, 0, nullptr, nullptr,
                                      nullptr, 0)));
        g.v_ready = g.v_epoch == g.xa_epoch;  // materialize() left v = Xa eta1 of this very inverse in g.v
        if (!g.v_ready)
          hipLaunchKernelGGL((k_trmv_lower<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Xa, mp, mp, (const T*)g.eta1,
                             g.Wbuf + Bq * mp);
        LAUNCHCHK(ctx);
        continue;
      }
      g.v_ready = false;
      // pre-factorisation part of aug_factor: -2*eta2 back into La if it holds a factor, extension rows [eta1' ; 0]
      if (g.la_state != 0 && !use_pro) {  // (with the prologue, -2 eta2 is formed inside the launch and never stored)
        hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)g.eta2, mp, mp, mp, g.La, mp, mp, mp,
                           T(1), T(-2));
      }
      if (nl > 1 && dag_nb == 0)  // the task graphs take [eta1' ; 0] from eta1 itself (erow / CholBatch::R): only the plain launches need it in E
        hipLaunchKernelGGL((k_set_ext_rows<T>), grid1(TILE * mp), dim3(256), 0, st(), g.Wbuf + Bq * mp, mp, mp,
                           (const T*)g.eta1);
      LAUNCHCHK(ctx);
    }
    // the augmented Cholesky factorisations of the remaining latents share their launches (independent chains overlap)
    {
      std::vector<int> todo;
      for (int l = 0; l < nl; ++l)
        if (!lat[l].via_inverse) todo.push_back(l);
      if (!todo.empty()) AGPCHK(timing_begin());
      // chunking: task graphs take as many problems per launch as the residency bound allows (balanced chunks, e.g. 8 latents
      // as 4 + 4); if not even one fits, all of them share per-column launches
      const int64_t ntl = mp / TILE, nel = Bq / TILE + 1;
      size_t chunk = CHOL_MAXB;
      if (dag_nb > 0 && !todo.empty()) {
        const size_t nchunks = (todo.size() + dag_nb - 1) / dag_nb;
        chunk = (todo.size() + nchunks - 1) / nchunks;
      }
      int64_t launches = 0;
      for (size_t l0 = 0; l0 < todo.size(); l0 += chunk) {
        const int nb = (int)std::min<size_t>(chunk, todo.size() - l0);
        CholBatch<T>& bt = merged_bt;
        bt = CholBatch<T>{};
        for (int q = 0; q < nb; ++q) {
          Latent& g = lat[todo[l0 + q]];
          bt.A[q] = g.La;
          bt.X[q] = g.Xa;
          bt.Dg[q] = g.DgA;
          bt.E[q] = g.Wbuf;
          bt.R[q] = g.eta1;
          g.la_state = 1;
          g.xa_valid = false;
        }
        SafeSrc<T>& src = merged_src;  // where the in-stream fallback of the task graph finds the inputs again
        src = SafeSrc<T>{};
        src.Bq = Bq;
        for (int q = 0; q < nb; ++q) {
          Latent& g = lat[todo[l0 + q]];
          src.kappa[q] = g.kappa;
          src.eta1[q] = g.eta1;
          src.eta2[q] = g.eta2;
        }
        if (nb == 1) {  // also writes the [eta1' ; 0] block when it falls back to per-column launches
          ProArgs<T> ph{};
          if (use_pro) {
            Latent& g0 = lat[0];
            ph.ldk = mp;
            ph.eta2 = g0.eta2;
            ph.ldm = mp;
            ph.eta1 = g0.eta1;
            if (pendp.on) {  // reduced statistics of a batch-parallel step
              ph.packed = stats + mp;
              ph.tred = stats;
              if (pendp.overlap) {
                ph.arrive = arrive_dev;
                ph.arrive_want = pendp.epoch;
                memcpy(ph.grp, ov_grp, sizeof(ph.grp));
              }
              ph.Kdim = 0;
              ph.Kinv = pendp.Kinv;
              ph.kinv_mu0 = pendp.kinv_mu0;
              ph.lr = pendp.lr;
            } else {
              ph.kap = pend.kap;
              ph.Kdim = pend.Bq;
              ph.w = pend.w;
              if (use_epi && s00_for.on && s00_for.kap == pend.kap && s00_for.w == pend.w && s00_for.K == pend.Bq)
                ph.pre = s00buf;  // prepared by the deferred launch just enqueued (run_deferred_safe)
              ph.r = pend.r;
              ph.Kinv = pend.Kinv;
              ph.kinv_mu0 = pend.kinv_mu0;
              ph.lr = pend.lr;
            }
          }
          EpiArgs<T> ea{};
          if (use_epi) {
            Latent& g0 = lat[0];
            // this launch writes r, w of THIS minibatch while its prologue reads the pending step's pair: alternate
            std::swap(rbuf, rbuf2);
            std::swap(wbuf, wbuf2);
            ea.on = 1;
            ea.B = B;
            ea.nslices = ns;
            ea.pk = g0.pk;
            ea.ldp = ldp;
            ea.kdiag = kvar(g0);
            ea.kd_ptr = g0.scales + D;
            ea.use_kt = g0.keep_last ? 1 : 0;
            ea.jitter = (T)jitter;
            ea.rho = (T)rho;
            ea.lp = lp;
            ea.y = (const T*)y;
            ea.idx = idx;
            ea.Kt = Kt;
            ea.muf = muf;
            ea.varf = varf;
            ea.cb = cbuf;
            ea.theta = theta;
            ea.r = rbuf;
            ea.w = wbuf;
            ea.flags = flags_dev;
            ea.lam = lam_dev;
            ea.gamma = gamma;
          }
          PotrfReq<T> rq{};
          rq.A = bt.A[0], rq.ld = mp, rq.n = mp, rq.X = bt.X[0], rq.ldx = mp, rq.Dg = bt.Dg[0], rq.E = bt.E[0], rq.lde = mp, rq.ne = nel;
          rq.info_dev = info_dev, rq.nvalid = m;
          rq.erow = lat[todo[l0]].eta1, rq.want_l = false, rq.safe = &src;
          rq.defer_safe = nl == 1;  // single latent: the row-statistics launch below carries the fallback (k_safe_rowstats)
          if (sync_step) rq.ssync = &ssync;
          if (use_pro) rq.pro = &ph;
          if (use_epi) rq.epi = &ea;
          AGPCHK(potrf_fused<T>(ctx, rq));
          s00_for.on = false;
          if (use_pro) {  // the launch has taken the pending step (had it been refused, the step would still be pending for flush())
            pend.on = pendp.on = pendp.overlap = false;
            n_prologue += 1;
          }
          merged_safe = rq.defer_safe;
          launches += dag_nb > 0 ? 1 : chol_launch_count(ntl, nel);
        } else {
          PotrfBatchReq<T> rq{};
          rq.bt = &bt, rq.nb = nb, rq.ld = mp, rq.n = mp, rq.ldx = mp, rq.lde = mp, rq.ne = nel, rq.info_dev = info_dev, rq.nvalid = m;
          if (dag_nb > 0) {
            rq.safe = &src;
            AGPCHK(potrf_dag_batch<T>(ctx, rq));
            launches += 1;
          } else {
            AGPCHK(potrf_fused_batch<T>(ctx, rq));
            launches += chol_launch_count(ntl, nel);
          }
        }
      }
      if (!todo.empty()) AGPCHK(timing_end(launches));
    }
    if (ssync.used) started_seq = ssync.ds.seq;
    if (rel_pending) {  // the release of the previous step's kappa buffers: this step's `started` number, or an event now
      slot_kind[rel_slot] = ssync.used ? 1 : 0;
      slot_seq[rel_slot] = ssync.ds.seq;
      if (!ssync.used) HIPCHK(ctx, hipEventRecord(step_done[rel_slot], st()));
      rel_pending = false;
    }
    for (int l0 = 0; l0 < nl; l0 += ROWSTATS_MAXB) {  // row statistics + local update of all latents in one launch
      const int nb = std::min(ROWSTATS_MAXB, nl - l0);
      RowstatsBatch<T> rb{};
      for (int q = 0; q < nb; ++q) {
        Latent& g = lat[l0 + q];
        rb.pk[q] = g.pk;
        rb.W[q] = g.Wbuf;
        rb.v[q] = (g.via_inverse && g.v_ready) ? g.v : g.Wbuf + Bq * mp;
        rb.kdiag[q] = kvar(g);
        rb.kd_ptr[q] = g.scales + D;
        rb.use_kt[q] = g.keep_last ? 1 : 0;
      }
      if (merged_safe) {  // nl == 1
        AGPCHK(ensure_safe_words<T>(ctx));
        const int64_t nt_ = mp / TILE, ne_ = Bq / TILE + 1;
        const int64_t most = std::max<int64_t>(nt_ + ne_ + nt_ * (nt_ + 1) / 2 + ne_ * nt_, (B + 7) / 8);
        const unsigned g1 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(safe_grid_cap(ctx), most));
        if (use_epi) {  // the rows are done inside the task graph: the fallback launch waits for the head of the next step
          sdef.on = true;
          sdef.bt = merged_bt;
          sdef.src = merged_src;
          sdef.rb = rb;
          sdef.ne = ne_;
          sdef.nt = nt_;
          sdef.B = B;
          sdef.ns = ns;
          sdef.rho = (T)rho;
          sdef.y = (const T*)y;
          sdef.idx = idx;
          sdef.r = rbuf;
          sdef.w = wbuf;
          sdef.grid = g1;
          sdef.trace = ctx->strace_last;
          continue;
        }
        hipLaunchKernelGGL((k_safe_rowstats<T>), dim3(g1), dim3(CHOL_THREADS), 0, st(), merged_bt, merged_src, mp, mp, mp, ne_, nt_,
                           info_dev, m, ctx->safe_bar, ctx->safe_retries, B, ns, rb, ldp, mp, mp, (T)jitter, (T)rho, lp, (const T*)y,
                           idx, Kt, muf, varf, cbuf, theta, rbuf, wbuf, flags_dev, (const T*)lam_dev, gamma);
        LAUNCHCHK(ctx);
        continue;
      }
      const dim3 grid((unsigned)((B * 64 + 255) / 256), (unsigned)nb);
      hipLaunchKernelGGL((k_rowstats_local<T>), grid, dim3(256), 0, st(), B, ns, rb, ldp, mp, mp, (T)jitter, (T)rho, lp,
                         (const T*)y, idx, Kt + l0 * Bp, muf + l0 * Bp, varf + l0 * Bp, cbuf + l0 * Bp, theta + l0 * Bp,
                         rbuf + l0 * Bp, wbuf + l0 * Bp, Bp, flags_dev, (const T*)lam_dev, gamma + l0 * Bp);
      LAUNCHCHK(ctx);
    }
    AGPCHK(lik_tail(y, idx, B, rho, fresh));
    x_last = x;
    y_last = y;
    idx_last = idx;
    B_last = B;
    ldx_last = ldx;
    rho_last = rho;
    if (fresh) {  // (whose kappa the buffers hold now: see ev_x)
      ev_x = x;
      ev_idx = idx;
      ev_B = B;
      ev_ldx = ldx;
    }
    if (lp.kind == AGP_LIK_MULTIOUTPUT) {
      if (!mo) {
        ctx->err = "multi-output handle: call agp_svgp_set_multioutput first";
        return AGP_ERR_INVALID;
      }
      if (mo_sharded) return publish_f(muf, varf, 1);  // the driver all-reduces `fall`, then agp_svgp_mo_mix
      AGPCHK(mo_local(y, idx, B, rho, !fresh, muf, varf));
    }
    return AGP_OK;
  }

  // ---- hyper-parameter / inducing-point gradient (see agp_hyper.h) ------------------------------------------------
  agp_status hyper_rule(int k_rule, double k_rho, int z_rule, double z_rho) override {
    for (int r : {k_rule, z_rule})
      if (r != AGP_OPT_ADAM && r != AGP_OPT_DESCENT && r != AGP_OPT_MOMENTUM) {
        ctx->err = "agp_svgp_hyper_rule: unknown optimiser rule";
        return AGP_ERR_INVALID;
      }
    hy_krule = k_rule;
    hy_krho = k_rho;
    hy_zrule = z_rule;
    hy_zrho = z_rho;
    return AGP_OK;
  }
  agp_status hyper_configure(int opt_k, double k_eta, int opt_z, double z_eta, double b1, double b2,
                             double eps) override {
    hy_k = opt_k != 0;
    hy_z = opt_z != 0;
    hy_keta = k_eta;
    hy_zeta = z_eta;
    hy_b1 = b1;
    hy_b2 = b2;
    hy_eps = eps;
    return AGP_OK;
  }

  agp_status hyper_alloc() {
    if (hyH1) return AGP_OK;
    if (D > HB_MAXD) {
      ctx->err = "hyper-gradient: input dimension D = " + std::to_string(D) + " is above the supported maximum of " +
                 std::to_string(HB_MAXD) + " (HB_MAXD, agp_hyper.h)";
      return AGP_ERR_UNSUPPORTED;
    }
    // (partial sums per RT x 64 tile of a backward pass: k_kernel_backward, HB_RT rows per workgroup)
    int64_t tiles = std::max((Bp / HB_RT) * (mp / TILE), (mp / HB_RT) * (mp / TILE));
    // (the streaming model's pass through K_a = k(Z_a, Z_a) has map x map entries: with more old inducing points than new ones it
    // has more tiles than either pass above)
    for (const auto& g : lat)
      if (g.on && !g.on_first) tiles = std::max(tiles, (g.map / HB_RT) * (g.map / TILE));
    hy_tiles = tiles;
    const int64_t rowt = std::max(Bp / HB_RT, mp / HB_RT);
    AGPCHK(dmalloc(ctx, &hyH1, Bp * mp));
    AGPCHK(dmalloc(ctx, &hyH2, Bp * mp));
    AGPCHK(dmalloc(ctx, &hyH3, Bp * mp));
    AGPCHK(dmalloc(ctx, &hy_gmu, Bp));
    AGPCHK(dmalloc(ctx, &hy_gs, Bp));
    AGPCHK(dmalloc(ctx, &hy_muf, Bp));
    AGPCHK(dmalloc(ctx, &hy_pZ, rowt * mp * D));
    AGPCHK(dmalloc(ctx, &hy_dZ, m * D));
    AGPCHK(dmalloc(ctx, &hy_pvar, tiles));
    AGPCHK(dmalloc(ctx, &hy_pscale, tiles * D));
    AGPCHK(dmalloc(ctx, &hy_g, 1 + D));
    // second set of partial sums: both backward passes are reduced by ONE launch (k_hyper_reduce2)
    AGPCHK(dmalloc(ctx, &hy_pZ2, rowt * mp * D));
    AGPCHK(dmalloc(ctx, &hy_pvar2, tiles));
    AGPCHK(dmalloc(ctx, &hy_pscale2, tiles * D));
    return AGP_OK;
  }

  // gradient of the hyper objective w.r.t. (variance, per-dimension scales, Z) of latent l, on the batch of the last step
  agp_status hypergrad(int l, double* dvar, double* dscale, void* dZ_out) override {
    if (l < 0 || l >= nl || !x_last || B_last <= 0) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    if (g.k.kind == AGP_K_EXPONENTIAL) {
      ctx->err = "hyper-gradient: ExponentialKernel is not differentiable at zero distance";
      return AGP_ERR_UNSUPPORTED;
    }
    AGPCHK(hyper_alloc());
    const int64_t B = B_last, Bq = rup64(B);
    const T rho = (T)rho_last;
    // round 4: H = G_kappa K^-1 comes from ONE product, kappa (Sigma K^-1), with the K^-1 Sigma that is formed on the way to Apred
    // (k_hyper_hk) -- not kappa Sigma followed by (.) K^-1.  The heteroscedastic model needs kappa Sigma itself (var_f under the
    // current posterior) and keeps the two products.
    const bool one_product = lp.kind != AGP_LIK_HETEROSCEDASTIC;
    // ... and G_K from ONE more, C (Sigma K^-1), when the factorisation launch inside materialize() took the pending natural-gradient
    // step as its prologue and left C = kappa' diag(w) kappa + K^-1 / 4 behind (aug_factor, k_hyper_gK_fused): no kappa' H, no Apred
    AGPCHK(refresh_K());
    AGPCHK(materialize(g));
    const bool gk_fused = one_product && g.C_valid && g.C_kap == g.kappa && !g.stale_on && !(g.on && !g.on_first);
    n_hgrad += 1;
    n_gk_fused += gk_fused ? 1 : 0;
    // K^-1 mu rides on the mean_f / g_mu / g_sigma launch (k_hyper_muf_gvec) when that launch exists and nothing else needs it first
    const bool fuse_a = one_product && !mo && !g.pred_valid;
    struct PredGuard {  // an error return between here and the fused launch must not leave K^-1 mu marked valid
      bool* flag = nullptr;
      ~PredGuard() {
        if (flag) *flag = false;
      }
    } pred_guard;
    if (fuse_a) {
      if (!g.apred) AGPCHK(dmalloc(ctx, &g.apred, mp));
      g.pred_valid = true;  // (ensure_pred below then skips its own launch)
      pred_guard.flag = &g.pred_valid;
    }
    AGPCHK(ensure_pred(g, !gk_fused));  // Sigma, mu, K^-1 mu (, Apred = K^-1 - K^-1 Sigma K^-1)
    // AGP_FLAG_STALE_K: the step's kappa mixes the new Knm with the frozen inv(K); the differentiated ELBO recomputes the
    // kernel matrices (ELBO.jl:15-21), so the gradient takes kappa = Knm K^-1 with the FRESH inverse
    if (g.stale_on && lp.kind == AGP_LIK_HETEROSCEDASTIC) {
      ctx->err = "reference_compat_stale_K is not wired for the heteroscedastic hyper-gradient";
      return AGP_ERR_UNSUPPORTED;
    }
    // (a full-batch AnalyticVI run does not even recompute Knm after a hyper step -- its kappa cache stays valid,
    //  training.jl:196-204 -- so there the gradient also needs Knm under the current kernel and Z)
    auto knm_for_grad = [&](Latent& q) -> const T* {
      if (!q.stale_on || desc.stochastic) return q.Knm;
      if (!hyKnm && dmalloc(ctx, &hyKnm, Bp * mp) != AGP_OK) return nullptr;
      dim3 gk((unsigned)(mp / TILE), (unsigned)(Bq / TILE));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)x_last, ldx_last, idx_last, B,
                         (const T*)q.Z, D, m, D, (const T*)q.scales, q.k.kind, kvar(q), hyKnm, mp, Bq, mp, 0, T(0),
                         (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)q.Zsc, (const T*)q.zn);
      return hyKnm;
    };
    auto kappa_for_grad = [&](Latent& q) -> const T* {
      if (!q.stale_on) return q.kappa;
      const T* kn = knm_for_grad(q);
      if (!kn) return nullptr;
      if (!hyKap && dmalloc(ctx, &hyKap, Bp * mp) != AGP_OK) return nullptr;
      if (gemm_nt<T, EPI_STORE>(ctx, kn, mp, q.Kinv, mp, Bq, mp, mp, 0, hyKap, mp, nullptr, 0, nullptr, nullptr, nullptr,
                                0) != AGP_OK)
        return nullptr;
      return hyKap;
    };
    const T* kap = kappa_for_grad(g);
    if (!kap) return AGP_ERR_NOMEM;
    // mean_f with the current posterior, then g_mu / g_sigma from the step's local variables
    if (!one_product || mo)
      hipLaunchKernelGGL((k_gemv_rows<T>), grid1(B * 64), dim3(256), 0, st(), kap, mp, B, mp, (const T*)g.mu, hy_muf);
    if (!one_product)
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, kap, mp, g.Sigma, mp, Bq, mp, mp, 0, hyH1, mp, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));
    if (mo) {
      // mixed means under the current posterior need every latent's mean_f on this batch
      if (mo_sharded && fall_state != 2) {
        ctx->err = "latent-sharded multi-output hyper-gradient: call agp_svgp_mo_refresh_f and all-reduce the exchange "
                   "buffer first";
        return AGP_ERR_INVALID;
      }
      for (int q = 0; q < nl && !mo_sharded; ++q) {
        AGPCHK(materialize(lat[q]));
        const T* kq = q == l ? kap : kappa_for_grad(lat[q]);
        if (!kq) return AGP_ERR_NOMEM;
        hipLaunchKernelGGL((k_gemv_rows<T>), grid1(B * 64), dim3(256), 0, st(), kq, mp, B, mp, (const T*)lat[q].mu,
                           emuf + q * Bp);
      }
      if (g.stale_on && nl > 1 && !mo_sharded) {  // the scratch now holds another latent's kappa
        kap = kappa_for_grad(g);
        if (!kap) return AGP_ERR_NOMEM;
      }
      hipLaunchKernelGGL((k_mo_hyper_gvec<T>), grid1(B), dim3(256), 0, st(), B, Qa(), Bp, mocfg, (const T*)A_dev,
                         (const T*)y_last, ystride, idx_last, mo_sharded ? (const T*)fall : (const T*)emuf,
                         (const T*)mo_th, l + qlo,
                         (int)(desc.elbo_mode == AGP_ELBO_REFERENCE), hy_gmu, hy_gs);
      LAUNCHCHK(ctx);
    } else {
      int gmode = 0;
      const bool refm = desc.elbo_mode == AGP_ELBO_REFERENCE;
      if (refm && (lp.kind == AGP_LIK_LOGISTIC || lp.kind == AGP_LIK_NEGBINOMIAL)) gmode = 1;
      if (refm && lp.kind == AGP_LIK_BAYESIANSVM) gmode = 2;
      if (lp.kind == AGP_LIK_HETEROSCEDASTIC && l == 0) {
        gmode = 3;  // needs var_f under the current posterior: rowdot(kappa Sigma, kappa) + K~
        hipLaunchKernelGGL((k_hyper_varf<T>), grid1(B * 64), dim3(256), 0, st(), B, mp, mp, (const T*)hyH1,
                           kap, (const T*)(Kt + l * Bp), pw0);
      }
      if (one_product) {
        hipLaunchKernelGGL((k_hyper_muf_gvec<T>), grid1((B + (fuse_a ? mp : 0)) * 64), dim3(256), 0, st(), B, mp, mp, rho, gmode,
                           kap, (const T*)g.mu, (const T*)(rbuf + l * Bp), (const T*)(theta + l * Bp), (const T*)y_last, idx_last,
                           hy_muf, hy_gmu, hy_gs, fuse_a ? (const T*)g.Kinv : (const T*)nullptr, g.apred);
        pred_guard.flag = nullptr;  // K^-1 mu is enqueued
      } else
        hipLaunchKernelGGL((k_hyper_gvec<T>), grid1(B), dim3(256), 0, st(), B, rho, gmode, (const T*)(rbuf + l * Bp),
                           (const T*)(theta + l * Bp), (const T*)hy_muf, (const T*)y_last, idx_last, (const T*)pw0,
                           (const T*)gamma, (const T*)lam_dev, hy_gmu, hy_gs);
      LAUNCHCHK(ctx);
    }
    const T* knm = knm_for_grad(g);  // (the scratch is per handle: recomputed after the loop over the other latents)
    if (!knm) return AGP_ERR_NOMEM;
    if (one_product) {
      if (tw2_kis_of != l) {  // Apred was still valid (a prediction since the last step): K^-1 Sigma is not in the scratch
        AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Kinv, mp, g.Sigma, mp, mp, mp, mp, 0, Tw2, mp, nullptr, 0, nullptr, nullptr,
                                      nullptr, 0)));
        tw2_kis_of = l;
      }
      if (gk_fused) {
        // kappa (K^-1 Sigma)' = kappa Sigma K^-1 with the element-wise pass behind it as the product's epilogue (EPI_HK): G_Knm and
        // the partial column sums of u = kappa' g_mu, two rows of partials per tile row (T1 itself is never stored)
        if (!hy_upart) AGPCHK(dmalloc(ctx, &hy_upart, 2 * (Bp / TILE) * mp));
        HkArgs<T> hk{};
        hk.gmu = hy_gmu;
        hk.gs = hy_gs;
        hk.rho = rho;
        hk.B = B;
        AGPCHK((gemm_nt<T, EPI_HK>(ctx, kap, mp, Tw2, mp, Bq, mp, mp, 0, (T*)nullptr, mp, kap, mp, (const T*)g.apred, hy_upart, hyH3,
                                   mp, &hk)));
      } else {
        AGPCHK((gemm_nt<T, EPI_STORE>(ctx, kap, mp, Tw2, mp, Bq, mp, mp, 0, hyH1, mp, nullptr, 0, nullptr, nullptr, nullptr,
                                      0)));  // kappa (K^-1 Sigma)' = kappa Sigma K^-1
        hipLaunchKernelGGL((k_hyper_hk<T>), grid2(Bq, mp), blk2, 0, st(), B, Bq, mp, mp, rho, (const T*)hy_gmu,
                           (const T*)hy_gs, (const T*)g.apred, (const T*)hyH1, kap, hyH2, hyH3);
      }
      LAUNCHCHK(ctx);
    } else {
      hipLaunchKernelGGL((k_hyper_gkappa<T>), grid2(Bq, mp), blk2, 0, st(), B, Bq, mp, mp, rho, (const T*)hy_gmu,
                         (const T*)hy_gs, (const T*)g.mu, knm, hyH1);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, hyH1, mp, g.Kinv, mp, Bq, mp, mp, 0, hyH2, mp, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));
      hipLaunchKernelGGL((k_hyper_gknm<T>), grid2(Bq, mp), blk2, 0, st(), B, Bq, mp, mp, rho, (const T*)hy_gs,
                         (const T*)hyH2, kap, hyH3);
    }
    if (gk_fused) {
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Cmat, mp, Tw2, mp, mp, mp, mp, 0, Tw, mp, nullptr, 0, nullptr, nullptr, nullptr,
                                    0)));  // C (K^-1 Sigma)' = C Sigma K^-1
      hipLaunchKernelGGL((k_hyper_gK_fused<T>), dim3((unsigned)(mp / 32), (unsigned)(mp / 32)), dim3(256), 0, st(), m, mp,
                         (const T*)Tw, (const T*)g.Cmat,
                         (const T*)g.Kinv, (const T*)g.apred, (const T*)g.kinv_mu0, (const T*)hy_upart, (int)(2 * (Bq / TILE)), mp, rho,
                         Tw2);
    } else {
      dim3 gt((unsigned)(mp / TILE), (unsigned)(mp / TILE));
      if ((mp / TILE) * (mp / TILE) <= 320)
        hipLaunchKernelGGL((k_gemm_tn<T, 2>), gt, dim3(2 * NTHREADS), 0, st(), kap, mp, (const T*)hyH2, mp, Bq, Tw, mp);
      else
        hipLaunchKernelGGL((k_gemm_tn<T, 1>), gt, dim3(NTHREADS), 0, st(), kap, mp, (const T*)hyH2, mp, Bq, Tw, mp);
      hipLaunchKernelGGL((k_hyper_gK<T>), grid2(mp, mp), blk2, 0, st(), m, mp, (const T*)Tw, (const T*)g.Apred,
                         (const T*)g.apred, Tw2, (T)(1.0 / (double)bs_world), (const T*)g.kinv_mu0);
    }
    tw2_kis_of = -1;
    // backward through kernelmatrix(k, x, Z)  (gradient w.r.t. the second argument); its reduction initialises the gradient and
    // adds the kdiag term of the variance (rho sum_i g_sigma,i), which used to be a memset in front and a kernel behind.  Unless the
    // streaming model's extra passes follow, the reductions of both backward passes are ONE launch behind the second pass
    // (k_hyper_reduce2, second set of partial sums).
    const bool online_x = g.on && !g.on_first;
    const bool one_reduce = !online_x;
    if (!one_reduce) {  // (one_reduce: this pass shares the launch of the pass through K_ZZ below, k_kernel_backward2)
      dim3 gk((unsigned)(mp / TILE), (unsigned)(Bq / HB_RT));
      const int64_t tiles = (int64_t)gk.x * gk.y;
      hipLaunchKernelGGL((k_kernel_backward<T>), gk, dim3(NTHREADS), 0, st(), (const T*)x_last, ldx_last, idx_last, B,
                         (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), (const T*)hyH3, mp,
                         hy_pvar, hy_pscale, hy_pZ, mp);
      hipLaunchKernelGGL((k_hyper_reduce<T>), dim3((unsigned)(D + 1 + (m * D + 255) / 256)), dim3(256), 0, st(), tiles, D,
                           (const double*)hy_pvar, (const double*)hy_pscale, hy_g, 1.0, 1, (int64_t)gk.y, m, mp, (const T*)hy_pZ,
                           hy_dZ, T(1), (const T*)hy_gs, B, (double)rho);
    }
    if (online_x && bs_world > 1) {
      ctx->err = "hyper-gradient of a streaming (online) model on a batch-sharded handle is not wired";
      return AGP_ERR_UNSUPPORTED;
    }
    if (online_x) {
      // -extraKL (KLdivergences.jl:30-54) is part of the differentiated ELBO; its kernel matrices K_ab, kappa_a, K~_a are
      // recomputed with the candidate kernel / Z by compute_kappa(::OnlineVarLatent):
      //   G_kappa_a = D kappa_a (Sigma + mu mu') - eta_a mu' - D K_ab/2 ; G_Kab = G_kappa_a K^-1 - D kappa_a/2 ;
      //   G_K -= sym(kappa_a' G_kappa_a K^-1) ; G_Ka = D/2
      const int64_t map = g.map, ma = g.ma;
      if (map / TILE > std::max(Bp / TILE, mp / TILE) || (map / TILE) * (map / HB_RT) > hy_tiles) {
        ctx->err = "online hyper-gradient: more old inducing points than the scratch was sized for";
        return AGP_ERR_UNSUPPORTED;
      }
      dim3 gam((unsigned)(mp / TILE), (unsigned)(map / TILE));
      hipLaunchKernelGGL((k_add_outer<T>), grid2(mp, mp), blk2, 0, st(), (const T*)g.Sigma, (const T*)g.mu, mp, m, Tw);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.kappa_a, mp, Tw, mp, map, mp, mp, 0, g.oh1, mp, nullptr, 0, nullptr, nullptr, nullptr,
                                    0)));                                                       // kappa_a (Sigma + mu mu')
      hipLaunchKernelGGL((k_gemm_tn<T, 1>), gam, dim3(NTHREADS), 0, st(), (const T*)g.invDa, map, (const T*)g.oh1, mp, map,
                         g.oh2, mp);                                                              // D (.)
      hipLaunchKernelGGL((k_gemm_tn<T, 1>), gam, dim3(NTHREADS), 0, st(), (const T*)g.invDa, map, (const T*)g.Kab, mp, map,
                         g.oh3, mp);                                                              // D K_ab
      hipLaunchKernelGGL((k_online_gkappa<T>), grid2(map, mp), blk2, 0, st(), ma, m, map, mp, mp, (const T*)g.peta1,
                         (const T*)g.mu, (const T*)g.oh3, g.oh2);                                 // G_kappa_a
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.oh2, mp, g.Kinv, mp, map, mp, mp, 0, g.oh1, mp, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));                                              // G_kappa_a K^-1
      {
        dim3 gmm((unsigned)(mp / TILE), (unsigned)(mp / TILE));
        hipLaunchKernelGGL((k_gemm_tn<T, 1>), gmm, dim3(NTHREADS), 0, st(), (const T*)g.kappa_a, mp, (const T*)g.oh1, mp, map,
                           Tw, mp);                                                               // kappa_a' (G_kappa_a K^-1)
      }
      hipLaunchKernelGGL((k_sub_sym<T>), grid2(m, m), blk2, 0, st(), Tw2, (const T*)Tw, mp, m);
      hipLaunchKernelGGL((k_gemm_tn<T, 1>), gam, dim3(NTHREADS), 0, st(), (const T*)g.invDa, map, (const T*)g.kappa_a, mp, map,
                         g.oh3, mp);                                                              // D kappa_a
      hipLaunchKernelGGL((k_axpy2d<T>), grid2(map, mp), blk2, 0, st(), map, mp, mp, T(-0.5), (const T*)g.oh3, g.oh1);  // G_Kab
      LAUNCHCHK(ctx);
    }
    // backward through kernelmatrix(k, Z) : both arguments are Z and G_K is symmetric -> twice the second-argument part
    {
      dim3 gk((unsigned)(mp / TILE), (unsigned)(mp / HB_RT));
      const int64_t tiles = (int64_t)gk.x * gk.y;
      if (one_reduce) {
        KbPass<T> pa{(const T*)x_last, ldx_last, idx_last, B, (const T*)hyH3, mp, hy_pvar, hy_pscale, hy_pZ};
        KbPass<T> pb{(const T*)g.Z, D, (const int64_t*)nullptr, m, (const T*)Tw2, mp, hy_pvar2, hy_pscale2, hy_pZ2};
        const int64_t ny1 = Bq / HB_RT;
        hipLaunchKernelGGL((k_kernel_backward2<T>), dim3(gk.x, (unsigned)(ny1 + gk.y)), dim3(NTHREADS), 0, st(), pa, pb, ny1,
                           (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), mp);
      } else
        hipLaunchKernelGGL((k_kernel_backward<T>), gk, dim3(NTHREADS), 0, st(), (const T*)g.Z, D, (const int64_t*)nullptr,
                           m, (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), (const T*)Tw2, mp, hy_pvar, hy_pscale,
                           hy_pZ, mp);
      if (one_reduce && hy_grad_on_device_only && hy_k && hy_z && D + 1 <= 256) {
        // the training loop's hyper step: the reduction rides on the optimiser launch (k_hyper_reduce2_adam, hyper_apply_one)
        red_def.on = true;
        red_def.latent = l;
        red_def.nt1 = (int64_t)(mp / TILE) * (Bq / HB_RT);
        red_def.nrow1 = (int64_t)(Bq / HB_RT);
        red_def.nt2 = tiles;
        red_def.nrow2 = (int64_t)gk.y;
        red_def.B = B;
        red_def.rho = (double)rho;
      } else if (one_reduce)
        hipLaunchKernelGGL((k_hyper_reduce2<T>), dim3((unsigned)(D + 1 + (m * D + 255) / 256)), dim3(256), 0, st(), D, hy_g, m, mp,
                           hy_dZ, (int64_t)(mp / TILE) * (Bq / HB_RT), (const double*)hy_pvar, (const double*)hy_pscale,
                           (int64_t)(Bq / HB_RT), (const T*)hy_pZ, tiles, (const double*)hy_pvar2, (const double*)hy_pscale2,
                           (int64_t)gk.y, (const T*)hy_pZ2, (const T*)hy_gs, B, (double)rho);
      else
        hipLaunchKernelGGL((k_hyper_reduce<T>), dim3((unsigned)(D + 1 + (m * D + 255) / 256)), dim3(256), 0, st(), tiles, D,
                           (const double*)hy_pvar, (const double*)hy_pscale, hy_g, 1.0, 0, (int64_t)gk.y, m, mp, (const T*)hy_pZ,
                           hy_dZ, T(2), (const T*)nullptr, (int64_t)0, 0.0);
    }
    if (online_x) {
      // K_ab = k(Z_a, Z): gradient w.r.t. the kernel parameters and the second argument ; K_a = k(Z_a, Z_a): parameters only
      const int64_t map = g.map, ma = g.ma;
      dim3 gk((unsigned)(mp / TILE), (unsigned)(map / HB_RT));
      hipLaunchKernelGGL((k_kernel_backward<T>), gk, dim3(NTHREADS), 0, st(), (const T*)g.Za, D, (const int64_t*)nullptr, ma,
                         (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), (const T*)g.oh1, mp, hy_pvar,
                         hy_pscale, hy_pZ, mp);
      hipLaunchKernelGGL((k_hyper_reduce_scalar<T>), dim3((unsigned)(D + 1)), dim3(256), 0, st(), (int64_t)gk.x * gk.y, D,
                         (const double*)hy_pvar, (const double*)hy_pscale, hy_g, 1.0);
      hipLaunchKernelGGL((k_hyper_reduce_Z<T>), grid1(m * D), dim3(256), 0, st(), (int64_t)gk.y, m, mp, D, (const T*)hy_pZ,
                         hy_dZ, T(1), 1);
      dim3 ga((unsigned)(map / TILE), (unsigned)(map / HB_RT));
      hipLaunchKernelGGL((k_kernel_backward<T>), ga, dim3(NTHREADS), 0, st(), (const T*)g.Za, D, (const int64_t*)nullptr, ma,
                         (const T*)g.Za, D, ma, D, (const T*)g.scales, g.k.kind, kvar(g), (const T*)g.invDa, map,
                         hy_pvar, hy_pscale, hy_pZ, (int64_t)0);  // (p_pad = 0: no pZ; map rows would not fit hy_pZ's mp)
      hipLaunchKernelGGL((k_hyper_reduce_scalar<T>), dim3((unsigned)(D + 1)), dim3(256), 0, st(), (int64_t)ga.x * ga.y, D,
                         (const double*)hy_pvar, (const double*)hy_pscale, hy_g, 0.5);
      LAUNCHCHK(ctx);
    }
    LAUNCHCHK(ctx);
    if (dZ_out) HIPCHK(ctx, hipMemcpyAsync(dZ_out, hy_dZ, sizeof(T) * m * D, hipMemcpyDeviceToDevice, st()));
    return hypergrad_to_host(dvar, dscale);
  }
  // hy_g -> dvar / dscale, hy_last (the training loop's hyper step keeps it on the device for ADAM: hy_grad_on_device_only)
  agp_status hypergrad_to_host(double* dvar, double* dscale) {
    if (hy_grad_on_device_only) return AGP_OK;
    std::vector<double> hg(1 + D);
    HIPCHK(ctx, hipMemcpyAsync(hg.data(), hy_g, sizeof(double) * (1 + D), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    if (dvar) *dvar = hg[0];
    if (dscale)
      for (int64_t d = 0; d < D; ++d) dscale[d] = hg[1 + d];
    hy_last = hg;
    return AGP_OK;
  }
  std::vector<double> hy_last;
  bool hy_grad_on_device_only = false;  // set around hypergrad() by hyper_step(): no download, no synchronisation
  struct RedDeferred {  // the gradient's final reduction, left to the optimiser launch (k_hyper_reduce2_adam)
    bool on = false;
    int latent = -1;
    int64_t nt1 = 0, nrow1 = 0, nt2 = 0, nrow2 = 0, B = 0;
    double rho = 0.0;
  } red_def;

  // ADAM moments of the kernel-parameter optimiser (1 + D entries: variance, scales; a ScaleTransform uses entry 1 only).  They
  // live on the device (Latent::kadam); this call copies them out / in (handle re-creation, the online model's chain of handles,
  // checkpoints) and synchronises.
  agp_status ensure_kadam(Latent& g) {
    if (!g.kadam) {
      AGPCHK(dmalloc(ctx, &g.kadam, 2 * (1 + D)));
      HIPCHK(ctx, hipMemsetAsync(g.kadam, 0, sizeof(double) * 2 * (1 + D), st()));
      g.k_step = 0;
    }
    return AGP_OK;
  }
  agp_status hyper_state(int l, int set, double* k_m, double* k_v, int32_t* k_step) override {
    if (l < 0 || l >= nl || !k_m || !k_v || !k_step) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    const size_t np = 1 + (g.k.ard ? (size_t)D : 1);
    AGPCHK(ensure_kadam(g));
    std::vector<double> h(2 * (1 + D), 0.0);
    if (set) {
      for (size_t i = 0; i < np; ++i) {
        h[i] = k_m[i];
        h[1 + D + i] = k_v[i];
      }
      HIPCHK(ctx, hipMemcpyAsync(g.kadam, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      g.k_step = *k_step;
    } else {
      HIPCHK(ctx, hipMemcpyAsync(h.data(), g.kadam, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      for (size_t i = 0; i < np; ++i) {
        k_m[i] = h[i];
        k_v[i] = h[1 + D + i];
      }
      *k_step = g.k_step;
    }
    return AGP_OK;
  }

  // ADAM ascent on latent l (update_kernel!, autotuning_utils.jl:47-67; update_Z!, :70-76) -- ON THE DEVICE, from the gradient in
  // hy_g = [dvariance, dscale_0..D-1] (doubles, w.r.t. the parameters themselves) and dZ_dev (m x D).  hg_host != nullptr: a
  // caller-supplied gradient (tied / all-reduced) is uploaded into hy_g first.  Nothing synchronises; the host copy of the kernel
  // parameters goes stale until somebody asks for it (params_to_host).
  agp_status hyper_apply_one(int l, const std::vector<double>* hg_host, const T* dZ_dev) {
    Latent& g = lat[l];
    const bool red_here = red_def.on && red_def.latent == l && !hg_host && dZ_dev == (const T*)hy_dZ;
    if (red_def.on && !red_here) {
      ctx->err = "hyper step: a deferred gradient reduction was not taken by its optimiser launch";
      red_def.on = false;
      return AGP_ERR_INVALID;
    }
    if (red_here) {  // reduction of both backward passes + both optimiser steps: ONE launch
      red_def.on = false;
      AGPCHK(hyper_alloc());
      AGPCHK(ensure_kadam(g));
      if (!g.z_am) {
        AGPCHK(dmalloc(ctx, &g.z_am, m * D));
        AGPCHK(dmalloc(ctx, &g.z_av, m * D));
        HIPCHK(ctx, hipMemsetAsync(g.z_am, 0, sizeof(double) * m * D, st()));
        HIPCHK(ctx, hipMemsetAsync(g.z_av, 0, sizeof(double) * m * D, st()));
      }
      g.k_step += 1;
      g.z_step += 1;
      const int64_t nzb = (m * D + HYPER_RA_THREADS - 1) / HYPER_RA_THREADS;
      hipLaunchKernelGGL((k_hyper_reduce2_adam<T>), dim3((unsigned)(nzb + 1)), dim3(HYPER_RA_THREADS), 0, st(), D, hy_g, m, mp, hy_dZ, red_def.nt1,
                         (const double*)hy_pvar, (const double*)hy_pscale, red_def.nrow1, (const T*)hy_pZ, red_def.nt2,
                         (const double*)hy_pvar2, (const double*)hy_pscale2, red_def.nrow2, (const T*)hy_pZ2, (const T*)hy_gs, red_def.B,
                         red_def.rho, g.Z, g.z_am, g.z_av, g.z_step, hy_zeta, hy_zrule, hy_zrho, g.k.ard ? 1 : 0,
                         g.k.has_variance ? 1 : 0, g.k.has_transform ? 1 : 0, g.scales, g.kadam, g.kadam + (1 + D), g.k_step, hy_keta,
                         hy_krule, hy_krho, hy_b1, hy_b2, hy_eps);
      LAUNCHCHK(ctx);
      g.host_params_stale = true;
      return AGP_OK;
    }
    if (hy_k && hy_z && dZ_dev && D + 1 <= 256) {  // both steps in one launch (k_adam_z_and_params)
      AGPCHK(hyper_alloc());
      AGPCHK(ensure_kadam(g));
      if (hg_host) {
        hy_up = *hg_host;  // staging that outlives the asynchronous copy
        HIPCHK(ctx, hipMemcpyAsync(hy_g, hy_up.data(), sizeof(double) * (1 + D), hipMemcpyHostToDevice, st()));
      }
      if (!g.z_am) {
        AGPCHK(dmalloc(ctx, &g.z_am, m * D));
        AGPCHK(dmalloc(ctx, &g.z_av, m * D));
        HIPCHK(ctx, hipMemsetAsync(g.z_am, 0, sizeof(double) * m * D, st()));
        HIPCHK(ctx, hipMemsetAsync(g.z_av, 0, sizeof(double) * m * D, st()));
      }
      g.k_step += 1;
      g.z_step += 1;
      const int64_t nzb = (m * D + 255) / 256;
      hipLaunchKernelGGL((k_adam_z_and_params<T>), dim3((unsigned)(nzb + 1)), dim3(256), 0, st(), m * D, nzb, g.Z, dZ_dev, g.z_am,
                         g.z_av, g.z_step, hy_zeta, hy_zrule, hy_zrho, (int)D, g.k.ard ? 1 : 0, g.k.has_variance ? 1 : 0,
                         g.k.has_transform ? 1 : 0, (const double*)hy_g, g.scales, g.kadam, g.kadam + (1 + D), g.k_step, hy_keta,
                         hy_krule, hy_krho, hy_b1, hy_b2, hy_eps);
      LAUNCHCHK(ctx);
      g.host_params_stale = true;
      return AGP_OK;
    }
    if (hy_k) {
      AGPCHK(hyper_alloc());
      AGPCHK(ensure_kadam(g));
      if (hg_host) {
        hy_up = *hg_host;  // staging that outlives the asynchronous copy
        HIPCHK(ctx, hipMemcpyAsync(hy_g, hy_up.data(), sizeof(double) * (1 + D), hipMemcpyHostToDevice, st()));
      }
      g.k_step += 1;
      hipLaunchKernelGGL((k_adam_kernel_params<T>), dim3(1), dim3(256), 0, st(), (int)D, g.k.ard ? 1 : 0, g.k.has_variance ? 1 : 0,
                         g.k.has_transform ? 1 : 0, (const double*)hy_g, g.scales, g.kadam, g.kadam + (1 + D), g.k_step, hy_keta,
                         hy_b1, hy_b2, hy_eps, hy_krule, hy_krho);
      LAUNCHCHK(ctx);
      g.host_params_stale = true;
    }
    if (hy_z && dZ_dev) {
      if (!g.z_am) {
        AGPCHK(dmalloc(ctx, &g.z_am, m * D));
        AGPCHK(dmalloc(ctx, &g.z_av, m * D));
        HIPCHK(ctx, hipMemsetAsync(g.z_am, 0, sizeof(double) * m * D, st()));
        HIPCHK(ctx, hipMemsetAsync(g.z_av, 0, sizeof(double) * m * D, st()));
      }
      g.z_step += 1;
      hipLaunchKernelGGL((k_adam_ascent<T>), grid1(m * D), dim3(256), 0, st(), m * D, g.Z, dZ_dev, g.z_am, g.z_av, g.z_step,
                         hy_zeta, hy_b1, hy_b2, hy_eps, hy_zrule, hy_zrho);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }
  std::vector<double> hy_up;

  agp_status hyper_finish() {
    for (auto& g : lat) {
      if (stale_mode() && !g.stale_on && !g.on && !g.K_stale) {
        // reference_compat_stale_K: freeze what the step uses before the kernel / Z move
        const int64_t mm = mp * mp;
        if (!g.sKinv) {
          AGPCHK(dmalloc(ctx, &g.sKinv, mm));
          AGPCHK(dmalloc(ctx, &g.sXk, mm));
        }
        HIPCHK(ctx, hipMemcpyAsync(g.sKinv, g.Kinv, sizeof(T) * mm, hipMemcpyDeviceToDevice, st()));
        HIPCHK(ctx, hipMemcpyAsync(g.sXk, g.Xk, sizeof(T) * mm, hipMemcpyDeviceToDevice, st()));
        if (g.kinv_mu0) {
          if (!g.skinv_mu0) AGPCHK(dmalloc(ctx, &g.skinv_mu0, mp));
          HIPCHK(ctx, hipMemcpyAsync(g.skinv_mu0, g.kinv_mu0, sizeof(T) * mp, hipMemcpyDeviceToDevice, st()));
        }
        AGPCHK(resolve_logdet(g));
        g.s_half_logdetK = g.half_logdetK;
        g.stale_on = true;
      }
      g.K_stale = true;  // (the kernel parameters were stepped in place on the device: nothing to upload)
      g.zsc_valid = false;
      // (the reference's full-batch path keeps its kernel matrices across a hyper step, training.jl:196-204)
      g.kappa_eval = false;
      if (!(g.stale_on && !desc.stochastic)) g.kappa_valid = false;
      g.pred_valid = g.predvar_valid = false;
    }
    pf_valid = false;
    return AGP_OK;
  }

  // update_hyperparameters!(m, state, x, y): ADAM ASCENT; positive kernel parameters are stepped in log space
  // (update_kernel!, autotuning_utils.jl:63-67), Z directly (update_Z!, :70-76).  K is refreshed before the next step.
  bool hyper_multi_ok = false;
  agp_status hyper_step() override {
    if (!hy_k && !hy_z) return AGP_OK;
    if (bs_world > 1 && !hyper_multi_ok) {
      // every rank would step its kernel / Z with the gradient of its own shard and the replicas would drift apart
      ctx->err = "batch-sharded handle: take the hyper step through agp_svgp_hyper_step_multi (the gradient is all-reduced)";
      return AGP_ERR_INVALID;
    }
    for (int l = 0; l < nl; ++l) {
      hy_grad_on_device_only = true;
      const agp_status hs = hypergrad(l, nullptr, nullptr, nullptr);
      hy_grad_on_device_only = false;
      //  hypergrad() marks the reduction as deferred BEFORE its last fallible calls (the online model's extra passes, a
      // launch check, a copy): an error exit must not leave the mark behind for the next, unrelated hyper_apply to trip over
      if (hs != AGP_OK) red_def.on = false;
      AGPCHK(hs);
      AGPCHK(hyper_apply_one(l, nullptr, (const T*)hy_dZ));
    }
    return hyper_finish();
  }

  // the optimiser step with a caller-supplied gradient (e.g. summed over latents / all-reduced over ranks: tied-Z mode)
  agp_status hyper_apply(int l, const double* dvar, const double* dscale, const void* dZ) override {
    if (l < 0 || l >= nl || !dvar || !dscale) return AGP_ERR_INVALID;
    if (!hy_k && !hy_z) return AGP_OK;
    std::vector<double> hg(1 + D);
    hg[0] = *dvar;
    for (int64_t d = 0; d < D; ++d) hg[1 + d] = dscale[d];
    AGPCHK(hyper_apply_one(l, &hg, (const T*)dZ));
    return hyper_finish();
  }

  agp_status get_kernel(int l, double* var, double* scales) override {
    if (l < 0 || l >= nl) return AGP_ERR_INVALID;
    AGPCHK(params_to_host(lat[l]));
    if (var) *var = lat[l].k.variance;
    if (scales)
      for (int64_t d = 0; d < D; ++d) scales[d] = lat[l].k.scales[d];
    return AGP_OK;
  }

  // MOSVGP(kernel, likelihoods, inference, Zs; Aoptimiser)  src/models/MOSVGP.jl:33-115 : install the task likelihoods,
  // the mixing weights A (n_task x n_latent, rows normalised by the caller like MOSVGP.jl:101-104) and the A optimiser.
  agp_status set_multioutput(int n_task, const agp_lik_desc* liks, const double* A_host, double eta, double b1,
                             double b2, double eps) override {
    if (lp.kind != AGP_LIK_MULTIOUTPUT || n_task <= 0 || n_task > MO_MAXT || !liks || !A_host) return AGP_ERR_INVALID;
    for (int t = 0; t < n_task; ++t) {
      const int tk = liks[t].kind;
      if (!(tk == AGP_LIK_GAUSSIAN || tk == AGP_LIK_LOGISTIC || tk == AGP_LIK_STUDENTT || tk == AGP_LIK_LAPLACE ||
            tk == AGP_LIK_BAYESIANSVM || tk == AGP_LIK_NEGBINOMIAL)) {
        ctx->err = "multi-output tasks support the Gaussian / Logistic / StudentT likelihoods on this path";
        return AGP_ERR_UNSUPPORTED;
      }
      if (tk == AGP_LIK_GAUSSIAN && liks[t].p1 > 0) {
        ctx->err = "GaussianLikelihood(...; opt_noise) is not wired as a multi-output task likelihood";
        return AGP_ERR_UNSUPPORTED;
      }
      mocfg.kind[t] = liks[t].kind;
      mocfg.p0[t] = (T)liks[t].p0;
      mocfg.p1[t] = (T)liks[t].p1;
    }
    nT = n_task;
    mocfg.nT = n_task;
    ystride = n_task;  // targets are point-major: y[i * n_task + t]
    a_eta = eta;
    a_b1 = b1;
    a_b2 = b2;
    a_eps = eps;
    a_step = 0;
    if (!A_dev) {
      AGPCHK(dmalloc(ctx, &A_dev, (int64_t)MO_MAXT * Qa()));
      AGPCHK(dmalloc(ctx, &gradA_dev, (int64_t)MO_MAXT * Qa()));
      AGPCHK(dmalloc(ctx, &am_dev, (int64_t)MO_MAXT * Qa()));
      AGPCHK(dmalloc(ctx, &av_dev, (int64_t)MO_MAXT * Qa()));
      if (mo_sharded) AGPCHK(dmalloc(ctx, &fall, (int64_t)2 * qtot * Bp));
      T** bv[] = {&mo_mixm, &mo_mixv, &mo_th, &mo_cc, &mo_th_save};
      for (auto p : bv) AGPCHK(dmalloc(ctx, p, (int64_t)MO_MAXT * Bp));
    }
    std::vector<T> ha((size_t)n_task * Qa());
    for (size_t i = 0; i < ha.size(); ++i) ha[i] = (T)A_host[i];
    HIPCHK(ctx, hipMemcpyAsync(A_dev, ha.data(), sizeof(T) * ha.size(), hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipMemsetAsync(am_dev, 0, sizeof(double) * MO_MAXT * Qa(), st()));
    HIPCHK(ctx, hipMemsetAsync(av_dev, 0, sizeof(double) * MO_MAXT * Qa(), st()));
    HIPCHK(ctx, hipMemsetAsync(mo_cc, 0, sizeof(T) * MO_MAXT * Bp, st()));
    // local variables before the first step (init_local_vars): theta = 1/sigma2 (Gaussian) or 0
    for (int t = 0; t < n_task; ++t)
      hipLaunchKernelGGL((k_fill<T>), grid1(Bp), dim3(256), 0, st(), mo_th + (int64_t)t * Bp, Bp,
                         liks[t].kind == AGP_LIK_GAUSSIAN ? (T)(1.0 / liks[t].p0) : T(0));
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st()));
    mo = true;
    return AGP_OK;
  }

  agp_status get_A(double* A_host) override {
    if (!mo || !A_host) return AGP_ERR_INVALID;
    std::vector<T> ha((size_t)nT * Qa());
    HIPCHK(ctx, hipMemcpyAsync(ha.data(), A_dev, sizeof(T) * ha.size(), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    for (size_t i = 0; i < ha.size(); ++i) A_host[i] = (double)ha[i];
    return AGP_OK;
  }

  // update_A! then the mixed local updates / gradients (update_parameters!(::MOSVGP), training.jl:153-158)
  // fm / fv: T[Qa][Bp] mean_f / var_f of ALL latents (the handle's own muf / varf, or the exchanged `fall` when sharded:
  // update_A! is then replicated on every rank, the gradients r / w are written for the owned latents only)
  agp_status mo_local(const void* y, const int64_t* idx, int64_t B, double rho, bool update_A, const T* fm,
                      const T* fv) {
    const int Q = Qa();
    if (update_A && a_eta > 0) {
      a_step += 1;
      hipLaunchKernelGGL((k_mo_gradA<T>), dim3((unsigned)Q, (unsigned)nT), dim3(256), 0, st(), B, Q, Bp, mocfg,
                         (const T*)A_dev, (const T*)y, ystride, idx, fm, fv, (const T*)mo_th, gradA_dev);
      hipLaunchKernelGGL((k_mo_applyA<T>), dim3(1), dim3(64), 0, st(), nT, Q, A_dev, (const double*)gradA_dev, am_dev,
                         av_dev, a_step, a_eta, a_b1, a_b2, a_eps);
    }
    hipLaunchKernelGGL((k_mo_local<T>), grid1(B), dim3(256), 0, st(), B, Q, Bp, mocfg, (const T*)A_dev, (T)rho,
                       (const T*)y, ystride, idx, fm, fv, mo_mixm, mo_mixv, mo_th, mo_cc, rbuf, wbuf, 1, qlo, nl);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }

  agp_status mo_shard(int q_total) override {
    if (lp.kind != AGP_LIK_MULTIOUTPUT || mo || q_total < desc.latent_offset + nl || desc.latent_offset < 0) {
      ctx->err = "agp_svgp_mo_shard: call before agp_svgp_set_multioutput with q_total >= latent_offset + n_latent";
      return AGP_ERR_INVALID;
    }
    mo_sharded = true;
    qtot = q_total;
    qlo = desc.latent_offset;
    return AGP_OK;
  }
  // own rows of (mean_f, var_f) into the exchange buffer, zeros elsewhere
  agp_status publish_f(const T* fm, const T* fv, int state) {
    HIPCHK(ctx, hipMemsetAsync(fall, 0, sizeof(T) * 2 * qtot * Bp, st()));
    HIPCHK(ctx, hipMemcpyAsync(fall + (int64_t)qlo * Bp, fm, sizeof(T) * nl * Bp, hipMemcpyDeviceToDevice, st()));
    HIPCHK(ctx, hipMemcpyAsync(fall + (int64_t)(qtot + qlo) * Bp, fv, sizeof(T) * nl * Bp, hipMemcpyDeviceToDevice, st()));
    fall_state = state;
    return AGP_OK;
  }
  agp_status mo_fbuf_ptr(void** p, int64_t* n) override {
    if (!mo_sharded || !fall || !p || !n) return AGP_ERR_INVALID;
    *p = fall;
    *n = (int64_t)2 * qtot * Bp;
    return AGP_OK;
  }
  agp_status mo_mix() override {
    if (!mo_sharded || !mo || fall_state != 1) {
      ctx->err = "agp_svgp_mo_mix: needs a latent-sharded multi-output handle right after agp_svgp_step_local";
      return AGP_ERR_INVALID;
    }
    fall_state = 3;
    return mo_local(y_last, idx_last, B_last, rho_last, true, fall, fall + (int64_t)qtot * Bp);
  }
  agp_status mo_refresh_f() override {
    if (!mo_sharded || !mo || B_last <= 0) return AGP_ERR_INVALID;
    AGPCHK(posterior_f(B_last));
    return publish_f(emuf, evarf, 2);
  }
  // mean_f / var_f of the owned latents on the last batch with the CURRENT posterior -> emuf / evarf (analyticVI.jl:260-266)
  virtual agp_status posterior_f(int64_t B) {
    const int64_t Bq = rup64(B);
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      HIPCHK(ctx, hipMemcpyAsync(g.Wbuf, g.kappa, sizeof(T) * Bq * mp, hipMemcpyDeviceToDevice, st()));
      AGPCHK(aug_factor(g, Bq, 1));
      HIPCHK(ctx, hipMemcpyAsync(g.v, g.Wbuf + Bq * mp, sizeof(T) * mp, hipMemcpyDeviceToDevice, st()));
      hipLaunchKernelGGL((k_w_rowstats<T>), grid1(B * 64), dim3(256), 0, st(), (const T*)g.Wbuf, mp, B, mp,
                         (const T*)g.v, pw0, pw1);
      hipLaunchKernelGGL((k_meanvar_finish<T>), grid1(B), dim3(256), 0, st(), B, 1, (const T*)pw0, (const T*)pw1, ldp,
                         (const T*)(Kt + l * Bp), emuf + l * Bp, evarf + l * Bp);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }

  // Knm / kappa of the NEXT minibatch on a second stream.  The targets are the alternate buffers, last read by the
  // step before the most recently enqueued one, so the prefetch only has to wait for that older step.
  agp_status prefetch(const void* x, int64_t ldx, const int64_t* idx, int64_t B) override {
    AGPCHK(check_batch(B));
    if (!x || !idx || ldx < D) return AGP_ERR_INVALID;
    for (auto& g : lat)
      if (g.K_stale) return AGP_OK;  // nothing sensible to prefetch against
    if (!pf_stream) {
      {
        // one latent: lowest priority -- the look-ahead GEMM must not take CUs from the latency-bound factorisation chain (C2 0.309
        // -> 0.336 ms with the highest).  Several latents: highest -- the batched task graph holds every CU with mostly waiting
        // workgroups for 0.6 ms and nl look-ahead pairs have to get through next to it; a starved look-ahead is what the main stream
        // then waits for (C4, 8 latents: 1.34 -> 1.21 ms).
        int lo = 0, hi = 0;
        HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
        int pr = nl > 1 ? hi : lo;
        HIPCHK(ctx, hipStreamCreateWithPriority(&pf_stream, hipStreamNonBlocking, pr));
      }
      HIPCHK(ctx, hipEventCreateWithFlags(&pf_done, hipEventDisableTiming));
      for (auto& e : step_done) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      HIPCHK(ctx, hipEventRecord(step_done[0], st()));
      HIPCHK(ctx, hipEventRecord(step_done[1], st()));
      {
        // hand-over word (AGP_PF_INKERNEL=0 keeps the event)
        const char* e = getenv("AGP_PF_INKERNEL");
        sig_state = -1;
        if (!(e && e[0] == '0')) {
          bool ok = true;
          for (auto& q : sig)
            ok = ok && hipExtMallocWithFlags((void**)&q, 8, hipMallocSignalMemory) == hipSuccess && hipMemset(q, 0, 8) == hipSuccess;
          if (ok) {
            // both streams must be able to run kernels at the same time (k_handshake, agp_chol.h)
            int32_t* hs = nullptr;
            ok = hipMalloc((void**)&hs, 4 * sizeof(int32_t)) == hipSuccess && hipMemset(hs, 0, 4 * sizeof(int32_t)) == hipSuccess;
            if (ok) {
              (void)hipStreamSynchronize(st());
              hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, pf_stream, hs, (const int32_t*)(hs + 1), hs + 2);
              hipLaunchKernelGGL(k_handshake, dim3(1), dim3(64), 0, st(), hs + 1, (const int32_t*)hs, hs + 3);
              int32_t res[4] = {0, 0, 0, 0};
              ok = hipStreamSynchronize(pf_stream) == hipSuccess && hipStreamSynchronize(st()) == hipSuccess &&
                   hipMemcpy(res, hs, sizeof(res), hipMemcpyDeviceToHost) == hipSuccess && res[2] == 1 && res[3] == 1;
            }
            if (hs) (void)hipFree(hs);
          }
          if (ok) sig_state = 1;
          else
            for (auto& q : sig) {
              if (q) (void)hipFree(q);
              q = nullptr;
            }
        }
        (void)hipGetLastError();
      }
      for (auto& g : lat) {
        AGPCHK(dmalloc(ctx, &g.Knm_alt, Bp * mp));
        AGPCHK(dmalloc(ctx, &g.kappa_alt, Bp * mp));
        AGPCHK(dmalloc(ctx, &g.kappa_old, Bp * mp));
        AGPCHK(dmalloc(ctx, &g.Wbuf_alt, (Bp + TILE) * mp));
        AGPCHK(dmalloc(ctx, &g.pk_alt, (2 * mp / TILE) * Bp));
      }
    }
    // the alternate buffers were "current" in the step before the last enqueued one
    if (slot_kind[step_parity] == 1) {
      hipLaunchKernelGGL(k_wait_ge, dim3(1), dim3(64), 0, pf_stream, (const int32_t*)sig[0], slot_seq[step_parity], info_dev);
      LAUNCHCHK(ctx);
    } else
      HIPCHK(ctx, hipStreamWaitEvent(pf_stream, step_done[step_parity], 0));
    const int64_t Bq = rup64(B);
    hipStream_t keep_stream = ctx->stream;
    agp_status rc = AGP_OK;
    // several latents (round 4): their (K_nm, kappa) pairs are independent, and one in-order stream runs them as 2 nl kernels of
    // exactly one workgroup per CU each, next to a task graph that holds most CUs -- every kernel boundary drains.  They are spread
    // over two streams (fork / join by events on the look-ahead's own streams, none on the step's); more streams take too much of
    // the chip from the task graph (measured at C4, 8 latents: 1 stream 1.186, 2: 1.088, 3: 1.41, 4: 1.34 ms).
    constexpr int pf_ways = 2;
    // (only next to the batched task graph: at C5 -- blocked factorisation, GEMMs of 4096 tiles -- two streams cost 13.5 -> 14.5 ms)
    const int ways = (nl > 1 && chol_use_dag(ctx, mp / TILE, Bq / TILE + 1, 2)) ? std::min<int>(pf_ways, nl) : 1;
    if (ways > 1) {
      if (!pf_side[0]) {
        int lo = 0, hi = 0;
        HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
        const int pr = hi;
        for (int q = 0; q < PF_SIDE; ++q) {
          HIPCHK(ctx, hipStreamCreateWithPriority(&pf_side[q], hipStreamNonBlocking, pr));
          HIPCHK(ctx, hipEventCreateWithFlags(&pf_join[q], hipEventDisableTiming));
        }
        HIPCHK(ctx, hipEventCreateWithFlags(&pf_fork, hipEventDisableTiming));
      }
      HIPCHK(ctx, hipEventRecord(pf_fork, pf_stream));
      for (int q = 0; q < ways - 1; ++q) HIPCHK(ctx, hipStreamWaitEvent(pf_side[q], pf_fork, 0));
    }
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      hipStream_t sl = (ways > 1 && l % ways) ? pf_side[l % ways - 1] : pf_stream;
      ctx->stream = sl;  // reuse the launch helpers on the look-ahead streams
      dim3 gk((unsigned)(mp / TILE), (unsigned)(Bq / TILE));
      (void)launch_kernelmatrix<T>(ctx, sl, (const T*)x, ldx, idx, B, (const T*)g.Z,
                         D, m, D, (const T*)g.scales, g.k.kind, kvar(g), g.Knm_alt, mp, Bq, mp, 0, T(0),
                         (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
      rc = gemm_nt<T, EPI_KAPPA>(ctx, g.Knm_alt, mp, kinv_kappa(g), mp, Bq, mp, mp, 0, g.kappa_alt, mp, g.Knm_alt, mp, nullptr,
                                 g.pk_alt, g.Wbuf_alt, ldp);
      if (rc != AGP_OK) break;
    }
    ctx->stream = keep_stream;
    AGPCHK(rc);
    for (int q = 0; q < ways - 1; ++q) {
      HIPCHK(ctx, hipEventRecord(pf_join[q], pf_side[q]));
      HIPCHK(ctx, hipStreamWaitEvent(pf_stream, pf_join[q], 0));
    }
    HIPCHK(ctx, hipEventRecord(pf_done, pf_stream));
    if (sig_state == 1) {
      pf_seq += 1;
      hipLaunchKernelGGL(k_set_sig, dim3(1), dim3(1), 0, pf_stream, sig[1], pf_seq);
      LAUNCHCHK(ctx);
    }
    pf_valid = true;
    pf_x = x;
    pf_idx = idx;
    pf_B = B;
    pf_ldx = ldx;
    return AGP_OK;
  }

  agp_status lsm_gamma() override {
    if (lp.kind != AGP_LIK_LOGISTICSOFTMAX) return AGP_OK;
    hipLaunchKernelGGL((k_lsm_gamma<T>), grid1(B_last), dim3(256), 0, st(), B_last, nl, Bp, (const T*)muf,
                       (const T*)cbuf, (const T*)alpha, (const T*)beta, gamma, gsum);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  agp_status lsm_alpha() override {
    if (lp.kind != AGP_LIK_LOGISTICSOFTMAX) return AGP_OK;
    hipLaunchKernelGGL((k_lsm_alpha<T>), grid1(B_last), dim3(256), 0, st(), B_last, (const T*)gsum, alpha);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  agp_status lsm_gsum_ptr(void** p, int64_t* n) override {
    *p = gsum;
    *n = B_last;
    return AGP_OK;
  }
  // k_elbo_terms is one instantiation per likelihood (no scratch under the 1024-thread register budget)
  agp_status launch_elbo_terms(int64_t B, int nlat, const LikParams<T>& lk, int lat_off, int add_global, const T* yv,
                               const int32_t* ycls, const int64_t* idx, const T* mf, const T* vf, const T* cv, const T* thv,
                               const T* gv, const T* av, const T* bv, double* outp, int64_t ystr) {
#define AGP_ELBO_CASE(K)                                                                                                        \
  case K:                                                                                                                       \
    hipLaunchKernelGGL((k_elbo_terms<T, K>), dim3(1), dim3(1024), 0, st(), B, nlat, Bp, lk, desc.elbo_mode, lat_off, add_global, \
                       yv, ycls, idx, mf, vf, cv, thv, gv, av, bv, outp, ystr, (const T*)lam_dev, (int)shard_once);              \
    break;
    switch (lk.kind) {
      AGP_ELBO_CASE(LIK_GAUSSIAN)
      AGP_ELBO_CASE(LIK_LOGISTIC)
      AGP_ELBO_CASE(LIK_STUDENTT)
      AGP_ELBO_CASE(LIK_LSM)
      AGP_ELBO_CASE(LIK_LAPLACE)
      AGP_ELBO_CASE(LIK_BSVM)
      AGP_ELBO_CASE(LIK_POISSON)
      AGP_ELBO_CASE(LIK_NEGBIN)
      AGP_ELBO_CASE(LIK_HETERO)
      default:
        ctx->err = "ELBO data terms: unknown likelihood kind";
        return AGP_ERR_INVALID;
    }
#undef AGP_ELBO_CASE
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  bool lsm_finished = false;  // k_lsm_fused has written theta, r, w of this step already
  agp_status lsm_local_all() override {
    if (lp.kind != AGP_LIK_LOGISTICSOFTMAX) return AGP_OK;
    if (nl > LSM_FUSED_MAXL) {
      for (int it = 0; it < 2; ++it) {  // logisticsoftmax.jl:65
        AGPCHK(lsm_gamma());
        AGPCHK(lsm_alpha());
      }
      return AGP_OK;
    }
    // one lane per (point, latent), LG = 2^ceil(log2 nl) lanes per point, 64 threads per workgroup: the 8 x 1024 values of a C4
    // update spread over 128 workgroups (the kernel is latency, not bandwidth)
#define AGP_LSM_LAUNCH(LG)                                                                                                   \
  hipLaunchKernelGGL((k_lsm_fused<T, LG>), dim3((unsigned)((B_last * LG + 63) / 64)), dim3(64), 0, st(), B_last, nl, Bp,      \
                     desc.latent_offset, (T)rho_last, (const int32_t*)y_last, idx_last, (const T*)muf, (const T*)cbuf, alpha, \
                     (const T*)beta, gamma, gsum, theta, rbuf, wbuf, (int)desc.lik.n_class, flags_dev)
    if (nl <= 1) AGP_LSM_LAUNCH(1);
    else if (nl <= 2) AGP_LSM_LAUNCH(2);
    else if (nl <= 4) AGP_LSM_LAUNCH(4);
    else if (nl <= 8) AGP_LSM_LAUNCH(8);
    else AGP_LSM_LAUNCH(16);
#undef AGP_LSM_LAUNCH
    LAUNCHCHK(ctx);
    lsm_finished = true;
    return AGP_OK;
  }
  agp_status lsm_finish() {
    if (lp.kind != AGP_LIK_LOGISTICSOFTMAX) return AGP_OK;
    if (lsm_finished) {
      lsm_finished = false;
      return AGP_OK;
    }
    hipLaunchKernelGGL((k_lsm_finish<T>), grid1(B_last), dim3(256), 0, st(), B_last, nl, Bp, desc.latent_offset,
                       (T)rho_last, (const int32_t*)y_last, idx_last, (const T*)cbuf, (const T*)gamma, theta, rbuf,
                       wbuf, (int)desc.lik.n_class, flags_dev);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }

  double* logdetK_dev = nullptr;  // [nl] log det of chol(K) diagonals (half log det K), fetched lazily (resolve_logdet)
  bool refresh_lazy = false;      // set around refresh_K() by the training loop's step_local
  agp_status resolve_logdet(Latent& g) {
    if (!g.logdet_pending) return AGP_OK;
    double hl = 0;
    HIPCHK(ctx, hipMemcpyAsync(&hl, logdetK_dev + (&g - lat.data()), sizeof(double), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    g.half_logdetK = hl;
    g.logdet_pending = false;
    return AGP_OK;
  }
  bool lam_deferred = false;  // set around step_local by the batch-sharded driver (see cavi_step_multi)
  agp_status lambda_finish_reduced() {
    if (lp.kind == AGP_LIK_GAUSSIAN) {  // the reduced sum and batch size: the same ADAM step on every rank
      const int nb = (int)((B_last + 255) / 256);
      hipLaunchKernelGGL((k_noise_finish<T>), dim3(1), dim3(256), 0, st(), 1, (const double*)(scal_dev + 60), 0.0,
                         (const double*)(scal_dev + 62), noise_eta, 0.9, 0.999, 1e-8, noise_adam, lam_dev);
      hipLaunchKernelGGL((k_gauss_grads<T>), dim3(nb), dim3(256), 0, st(), B_last, (T)rho_last, (const T*)y_last, idx_last,
                         (const T*)lam_dev, theta, cbuf, rbuf, wbuf);
      LAUNCHCHK(ctx);
      return AGP_OK;
    }
    const int mode = lp.kind == AGP_LIK_POISSON ? 0 : 1;
    hipLaunchKernelGGL((k_lambda_finish_red<T>), dim3(1), dim3(64), 0, st(), (const double*)(scal_dev + 60), mode, lam_dev);
    if (lp.kind == AGP_LIK_HETEROSCEDASTIC) {
      const int nb = (int)((B_last + 255) / 256);
      hipLaunchKernelGGL((k_hetero_grads<T>), dim3(nb), dim3(256), 0, st(), B_last, Bp, (T)rho_last, (const T*)y_last, idx_last,
                         (const T*)lam_dev, (const T*)gamma, theta, rbuf, wbuf);
    }
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  double cur_lr() const {  // optimisers.jl:14-19 ; Descent(1.0) for AnalyticVI
    return desc.stochastic ? 1.0 / std::pow(desc.rm_tau + (double)n_opt, desc.rm_kappa) : 1.0;
  }

  // batch statistics ; fused: eta1/eta2 are stepped directly, otherwise stats = [t | S] for an all-reduce
  agp_status step_stats(bool fused) override {
    AGPCHK(lsm_finish());
    const int64_t Bq = rup64(B_last);
    const T lr = (T)cur_lr();
    if (fused && nl > 1 && nl <= SYRK_MAXB) {
      // all latents of the handle in ONE launch (blockIdx.y = latent): a single latent's tiles fill about half the chip
      SyrkBatch<T> b{};
      for (int l = 0; l < nl; ++l) {
        Latent& g = lat[l];
        b.A[l] = g.kappa;
        b.w[l] = wbuf + l * Bp;
        b.out[l] = g.La;
        b.eta2[l] = g.eta2;
        b.Kinv[l] = kinv_step(g);
        b.rvec[l] = rbuf + l * Bp;
        b.eta1[l] = g.eta1;
        b.kinv_mu0[l] = kinv_mu0_step(g);
      }
      const int64_t nt = mp / TILE, tiles = nt * (nt + 1) / 2, nrider = nt;
      T* fillp = nullptr;
      int64_t fused_used = 0, fstride = 0, nfill = 0;
      int fnb = 0;
      if (ctx->h_dirty[0].on && ctx->htype == (int)sizeof(T)) {  // hand-over refill riders, as in syrk_tn()
        fillp = (T*)ctx->hset[0];
        fused_used = ctx->h_dirty[0].used;
        fstride = ctx->h_dirty[0].stride;
        fnb = ctx->h_dirty[0].nb;
        nfill = 96;
        ctx->h_dirty[0].on = false;
      }
      const bool kg2 = tiles * nl <= kg2_limit() && Bq >= 4 * BK;
      dim3 grid((unsigned)(tiles + nrider + nfill), (unsigned)nl);
      if (kg2)
        hipLaunchKernelGGL((k_syrk_eta_batch<T, 2>), grid, dim3(2 * NTHREADS), 0, st(), b, mp, Bq, mp, mp, lr, tiles, nrider, fillp,
                           fused_used, fstride, fnb);
      else
        hipLaunchKernelGGL((k_syrk_eta_batch<T, 1>), grid, dim3(NTHREADS), 0, st(), b, mp, Bq, mp, mp, lr, tiles, nrider, fillp,
                           fused_used, fstride, fnb);
      LAUNCHCHK(ctx);
      return AGP_OK;
    }
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      T* sl = stats + l * stats_stride();
      if (fused) {  // one launch: eta2 step on the lower tiles, eta1 step on nt rider workgroups
        AGPCHK((syrk_tn<T, SY_ETA2>(ctx, g.kappa, mp, mp, Bq, wbuf + l * Bp, 0, g.La, mp, g.eta2,
                                    kinv_step(g), mp, lr, (const T*)(rbuf + l * Bp), g.eta1, kinv_mu0_step(g))));
      } else {
        // ONE launch: the packed lower tiles of kappa' diag(w) kappa, t = kappa' (rho g1) by rider workgroups (the same riders
        // as the fused step, so a one-rank run sums in the same order), and the hand-over refill in its shadow
        AGPCHK((syrk_tn<T, SY_PACK>(ctx, g.kappa, mp, mp, Bq, wbuf + l * Bp, 0, sl + mp, mp, (T*)nullptr,
                                    (const T*)nullptr, (int64_t)0, T(0), (const T*)(rbuf + l * Bp), sl, (const T*)nullptr)));
      }
      LAUNCHCHK(ctx);
    }
    if (!fused) AGPCHK(kappa_released());
    return AGP_OK;
  }
  agp_status stats_ptr(void** p, int64_t* n) override {
    *p = stats;
    *n = (int64_t)nl * stats_stride();
    return AGP_OK;
  }
#ifdef AGP_DEBUG_PTRS
  void* debug_ptr(int what) override {
    Latent& g = lat[0];
    switch (what) {
      case 0: return g.eta2;
      case 1: return g.eta1;
      case 2: return wbuf;
      case 3: return rbuf;
      case 4: return wbuf2;
      case 5: return rbuf2;
      case 6: return g.kappa;
      case 7: return g.Wbuf;
      case 8: return theta;
      default: return nullptr;
    }
  }
#endif

  // AGP_HYPER_GK_FUSED=0: the hyper-gradient forms G_K from kappa' H and Apred as before round 4 (A/B, tests)
  static bool gk_fused_on() {
    static const bool on = [] {
      const char* e = getenv("AGP_HYPER_GK_FUSED");
      return !(e && e[0] == '0');
    }();
    return on;
  }
  // Augmented Cholesky of -2*eta2 with the extension rows [kappa (Bq rows, already in Wbuf) ; eta1'] :
  //   Wbuf <- [kappa L^-T ; (L^-1 eta1)']   i.e. W and v of mean_f = W v, var_f = rowsum(W^2) + K~.
  // with_x additionally forms Xa = L^-1 (needed only for Sigma / mu export, ELBO and prediction).
  // tail (materialize): the caller's next launch carries the task graph's fallback itself (k_safe_symv_trmv) -- filled when it has to
  struct SafeTail {
    bool on = false;
    CholBatch<T> bt{};
    SafeSrc<T> src{};
    int64_t ne = 0, nt = 0;
  };
  agp_status aug_factor(Latent& g, int64_t Bq, int with_x, SafeTail* tail = nullptr) {
    // a pending natural-gradient step (only the hyper step's wrapper leaves one: every other entry point has flushed) rides on this
    // launch as its prologue -- the hyper-parameter iteration's "eta step, then factor the new -2 eta2 with its inverse" in ONE launch
    AGPCHK(run_deferred_safe());
    if (pendp.on) AGPCHK(flush());
    g.C_valid = false;
    ProArgs<T> ph{};
    bool use_pro = false;
    if (pend.on) {
      use_pro = nl == 1 && pro_allowed() && chol_use_dag(ctx, mp / TILE, Bq / TILE + 1) &&
                pend.Bq >= TILE && mp / TILE > 1;
      if (!use_pro) AGPCHK(flush());
    }
    if (use_pro) {
      ph.kap = pend.kap;
      ph.ldk = mp;
      ph.Kdim = pend.Bq;
      ph.w = pend.w;
      ph.r = pend.r;
      ph.eta2 = g.eta2;
      ph.Kinv = pend.Kinv;
      ph.ldm = mp;
      ph.eta1 = g.eta1;
      ph.kinv_mu0 = pend.kinv_mu0;
      ph.lr = pend.lr;
      // the hyper-parameter iteration's launch (the inverse rides along): leave C = S + K^-1 / 4 for the gradient's G_K (hypergrad)
      if (with_x && (hy_k || hy_z) && gk_fused_on() && !g.stale_on && !g.on && bs_world == 1 && !mo &&
          lp.kind != AGP_LIK_HETEROSCEDASTIC) {
        if (!g.Cmat) AGPCHK(dmalloc(ctx, &g.Cmat, mp * mp));
        ph.Cout = g.Cmat;
      }
    } else if (g.la_state != 0) {  // La holds a factor: rebuild -2*eta2
      hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)g.eta2, mp, mp, mp, g.La, mp, mp, mp,
                         T(1), T(-2));
      LAUNCHCHK(ctx);
    }
    AGPCHK(timing_begin());
    SafeSrc<T> src{};
    src.Bq = Bq;
    src.kappa[0] = g.kappa;  // every caller copies kappa into Wbuf first (or passes Bq = 0)
    src.eta1[0] = g.eta1;
    src.eta2[0] = g.eta2;
    // with_x: the inverse rides along (identity block rows of the task graph); its fallback forms X = L^-1 in the stream as well
    // (SafeSrc::want_x), so that no host check -- no stream synchronisation -- sits behind the launch (round 3: the hyper-parameter
    // iteration used to wait here once per step)
    src.want_x = with_x ? 1 : 0;
    PotrfReq<T> rq{};
    rq.A = g.La, rq.ld = mp, rq.n = mp, rq.X = g.Xa, rq.ldx = mp, rq.Dg = g.DgA, rq.E = g.Wbuf, rq.lde = mp, rq.ne = Bq / TILE + 1;
    rq.do_x = with_x, rq.info_dev = info_dev, rq.nvalid = m;
    rq.erow = g.eta1, rq.want_l = false, rq.safe = &src, rq.defer_safe = tail != nullptr;
    if (use_pro) rq.pro = &ph;
    // with_x: Sigma = Xa' Xa is what every caller forms next -- product workgroups at the end of the same task-graph launch do it
    if (with_x) rq.Pout = g.Sigma;
    AGPCHK(potrf_fused<T>(ctx, rq));
    const bool sigma_done = rq.p_done;
    if (tail) {
      tail->on = rq.defer_safe;
      if (rq.defer_safe) {
        tail->bt = CholBatch<T>{};
        tail->bt.A[0] = g.La;
        tail->bt.X[0] = g.Xa;
        tail->bt.Dg[0] = g.DgA;
        tail->bt.E[0] = g.Wbuf;
        tail->src = src;
        tail->ne = Bq / TILE + 1;
        tail->nt = mp / TILE;
      }
    }
    if (use_pro) {  // taken by the launch (a refused launch leaves it pending for flush())
      pend.on = false;
      s00_for.on = false;
      n_prologue += 1;
      if (ph.Cout) {
        g.C_valid = true;
        g.C_kap = ph.kap;
      }
    }
    AGPCHK(timing_end(chol_use_dag(ctx, mp / TILE, Bq / TILE + 1) ? 1 : chol_launch_count(mp / TILE, Bq / TILE + 1)));
    g.la_state = 1;
    g.xa_valid = with_x != 0;
    if (with_x) g.xa_epoch += 1;
    g.sigma_epoch = sigma_done ? g.xa_epoch : -1;
    return AGP_OK;
  }

  // after eta changed outside a step (set_state): La = -2*eta2 is (re)built lazily; validate it is SPD now
  agp_status refactor(Latent& g) {
    g.la_state = 1;  // force the rebuild from eta2
    g.post_valid = false;
    g.pred_valid = g.predvar_valid = false;
    AGPCHK(aug_factor(g, 0, 1));
    return AGP_OK;
  }

  agp_status step_global(bool fused) override {
    const T lr = (T)cur_lr();
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      if (!fused) {
        const T* sl = stats + l * stats_stride();
        const int64_t ntri = (mp / TILE) * (mp / TILE + 1) / 2;
        hipLaunchKernelGGL((k_eta2_from_packed<T>), dim3((unsigned)(4 * ntri + (mp + 255) / 256)), dim3(256), 0, st(), sl + mp, mp,
                           g.eta2, kinv_step(g), g.La, lr, ntri, sl, kinv_mu0_step(g), g.eta1, mp);
        LAUNCHCHK(ctx);
      }
      g.la_state = 0;  // La now holds the new -2*eta2 (unfactored); it is factored inside the next local phase
      g.xa_valid = false;
      g.C_valid = false;
      g.post_valid = false;
      g.pred_valid = g.predvar_valid = false;
    }
    n_opt += 1;
    if (fused) AGPCHK(kappa_released());
    return AGP_OK;
  }
  // marks the last use of this step's kappa buffers (they become the next prefetch target): after the fused step, or -- phase-split
  // path -- right after the packed statistics, so that the next look-ahead does not wait for the all-reduce and the eta step
  agp_status kappa_released() {
    if (pf_stream) {
      if (rel_pending) {  // (two releases without a step in between: cannot happen through the ABI's step sequence, but be safe)
        slot_kind[rel_slot] = 0;
        HIPCHK(ctx, hipEventRecord(step_done[rel_slot], st()));
        rel_pending = false;
      }
      step_parity ^= 1;
      if (sig_state == 1 && nl == 1) {  // decided when the next step is enqueued (step_local)
        rel_pending = true;
        rel_slot = step_parity ^ 1;
      } else {
        // (the step's deferred fallback, if it re-runs, rewrites the step's Wbuf and reads its pk: before the event releases them;
        //  it also prepares the head of the next launch, as the word protocol's deferred launch would -- ProArgs::pre -- in case
        //  that launch takes the pending step: the trajectory must not depend on the protocol)
        AGPCHK(run_deferred_safe(nullptr, 0, true));
        slot_kind[step_parity ^ 1] = 0;
        HIPCHK(ctx, hipEventRecord(step_done[step_parity ^ 1], st()));
      }
    }
    return AGP_OK;
  }

  agp_status check_status() override {
    int32_t words[4] = {0, 0, 0, 0};  // info | infoK | flags | orderK (k_logdiag_sum: did K_ZZ fail before or after the others?)
    HIPCHK(ctx, hipMemcpyAsync(words, info_dev, sizeof(words), hipMemcpyDeviceToHost, st()));
    int32_t acq_bad = 0;  // a bordering pivot of the pending points that was not positive and finite (agp_acq_batch.h)
    if (acqd.acqb.bad) HIPCHK(ctx, hipMemcpyAsync(&acq_bad, acqd.acqb.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st()));
    int32_t acqj_bad = 0;  // a Cholesky pivot of a joint batch's covariance that was not positive and finite (agp_acq_joint.h)
    if (acqjd.acqj.bad) HIPCHK(ctx, hipMemcpyAsync(&acqj_bad, acqjd.acqj.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    if (acq_bad != 0) HIPCHK(ctx, hipMemsetAsync(acqd.acqb.bad, 0, sizeof(int32_t), st()));
    if (acqj_bad != 0) HIPCHK(ctx, hipMemsetAsync(acqjd.acqj.bad, 0, sizeof(int32_t), st()));
    const int32_t info = words[0], infoK = words[1], orderK = words[3];
    const int flags = (int)words[2];
    dag_retry_check(ctx);  // steps the in-stream fallback had to re-run: warn once, stop using the task graph
    if (info != 0 || flags != 0) {
      HIPCHK(ctx, hipMemsetAsync(info_dev, 0, sizeof(int32_t), st()));
      HIPCHK(ctx, hipMemsetAsync(flags_dev, 0, sizeof(int), st()));
    }
    if (infoK != 0) HIPCHK(ctx, hipMemsetAsync(infoK_dev, 0, sizeof(int32_t), st()));
    if (orderK != 0) HIPCHK(ctx, hipMemsetAsync(info_dev + 3, 0, sizeof(int32_t), st()));
    // a non-SPD K_ZZ latched by a refresh inside the training loop is the ROOT cause of whatever followed it on a garbage inverse
    // (negative K~, NaNs, a non-SPD -2 eta2): it is reported first, like the PosDefException the reference raises at that refresh --
    // unless an earlier step had ALREADY latched a failure of its own when K_ZZ failed (orderK == 2: e.g. the stale-K quirk drives
    // K~ negative, the NaNs that follow reach the kernel parameters, and K_ZZ is the consequence), which then comes first below
    if (infoK > 0 && orderK != 2) {
      for (auto& q : lat) q.K_stale = true;
      ctx->err = "PosDefException: K_ZZ + jitter*I is not positive definite; leading minor " + std::to_string(infoK);
      return AGP_ERR_NOT_POSDEF;
    }
    if (flags & FLAG_NEG_KTILDE) {
      ctx->err = "K~ has negative values";  // latentgp.jl:213
      return AGP_ERR_NEG_KTILDE;
    }
    if (flags & FLAG_BAD_LABEL) {
      ctx->err = "class label outside the likelihood's classes";  // multiclass.jl:81-83
      return AGP_ERR_LABELS;
    }
    if (flags & FLAG_BAD_COUNT) {
      ctx->err = "Gibbs sampling: the targets of a NegBinomial likelihood must be non-negative integers (PolyaGamma(y + r, |f|))";
      return AGP_ERR_LABELS;
    }
    if (flags & FLAG_RNG_BOUND) {
      ctx->err = "Gibbs sampling: a variate sampler ran into its iteration bound (agp_rand.h); the chain is not valid from there";
      return AGP_ERR_HIP;
    }
    if (info == -2) {
      ctx->err = "the look-ahead stream waited about a minute for a CAVI step that never started (k_wait_ge)";
      return AGP_ERR_HIP;
    }
    if (info == -3) {  // (grid_barrier, agp_chol.h: a bounded wait since round 6 -- this used to be a hang)
      if (ctx->safe_bar) HIPCHK(ctx, hipMemsetAsync(ctx->safe_bar, 0, 2 * sizeof(unsigned), st()));
      dag_pause(ctx);
      ctx->err = "the in-stream fallback of an aborted task-graph launch could not complete: one of its workgroups did not become "
                 "resident within the grid barrier's limit (is another process holding compute units of this GPU?); the step's "
                 "results are not valid";
      return AGP_ERR_HIP;
    }
    if (info == -4) {
      ctx->err = "AGP_SPLIT_OVERLAP: a column group of the all-reduced statistics did not arrive within the gate's limit";
      return AGP_ERR_HIP;
    }
    if (info < 0) {
      ctx->err = "task-graph factorisation aborted: a tile dependency never arrived (spin limit)";
      return AGP_ERR_HIP;
    }
    if (info != 0) {
      ctx->err = "PosDefException: -2*eta2 is not positive definite; leading minor " + std::to_string(info);
      return AGP_ERR_NOT_POSDEF;
    }
    if (infoK > 0) {
      for (auto& q : lat) q.K_stale = true;
      ctx->err = "PosDefException: K_ZZ + jitter*I is not positive definite; leading minor " + std::to_string(infoK);
      return AGP_ERR_NOT_POSDEF;
    }
    if (infoK < 0) {
      ctx->err = "task-graph factorisation of K_ZZ aborted: a tile dependency never arrived (spin limit)";
      return AGP_ERR_HIP;
    }
    if (acq_bad != 0) {  // (last: whatever stands above made the predictor it was computed from)
      ctx->err = "PosDefException: the covariance of the pending points (agp_svgp_acquisition_pending, agp_svgp_acq_maximize_batch) is "
                 "not positive definite: a bordering pivot c was not positive and finite";
      return AGP_ERR_NOT_POSDEF;
    }
    if (acqj_bad != 0) {
      ctx->err = "PosDefException: the joint covariance of a batch (agp_svgp_acquisition_joint, agp_svgp_acq_maximize_joint) is not "
                 "positive definite: a Cholesky pivot was not positive and finite";
      return AGP_ERR_NOT_POSDEF;
    }
    return AGP_OK;
  }

  // Sigma = Xa' Xa ; mu = Xa' v   with Xa = chol(-2 eta2)^-1, v = Xa eta1     (inference.jl:25-28)
  agp_status materialize(Latent& g) {
    if (g.post_valid) return AGP_OK;
    SafeTail tail;
    if (!(g.la_state == 1 && g.xa_valid)) AGPCHK(aug_factor(g, 0, 1, &tail));
    if (tw2_kis_of == (int)(&g - lat.data())) tw2_kis_of = -1;  // K^-1 Sigma in the scratch belongs to the Sigma before this one
    if (g.sigma_epoch != g.xa_epoch) {  // (else: left by the launch itself)
      if (tail.on) {
        AGPCHK(launch_chol_safe<T>(ctx, tail.bt, tail.src, 1, mp, mp, mp, tail.ne, tail.nt, info_dev, m));
        tail.on = false;
      }
      AGPCHK(xtx_padded<T>(ctx, g.Xa, mp, mp, g.Sigma, mp));
    }
    // mu = Sigma eta1 as the reference writes it (global_update!, analyticVI.jl:229-246).  Until round 4 this was Xa' (Xa eta1) from
    // the factorisation's [eta1'] row: a copy and a 16-workgroup triangular mat-vec (4.8 + 15.6 us at m = 1024 against 7.0)
    if (tail.on) {  // the task graph's fallback rides on this launch
      AGPCHK(ensure_safe_words<T>(ctx));
      const int64_t most = std::max<int64_t>(tail.nt + tail.ne + tail.nt * (tail.nt + 1) / 2 + tail.ne * tail.nt, (2 * mp + 7) / 8);
      const unsigned g1 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(safe_grid_cap(ctx), most));
      hipLaunchKernelGGL((k_safe_symv_trmv<T>), dim3(g1), dim3(CHOL_THREADS), 0, st(), tail.bt, tail.src, mp, mp, mp, tail.ne, tail.nt,
                         info_dev, m, ctx->safe_bar, ctx->safe_retries, (const T*)g.Sigma, (const T*)g.Xa, mp, mp, (const T*)g.eta1,
                         g.mu, g.v);
    } else
      hipLaunchKernelGGL((k_symv_trmv<T>), grid1(2 * mp * 64), dim3(256), 0, st(), (const T*)g.Sigma, (const T*)g.Xa, mp, mp,
                         (const T*)g.eta1, g.mu, g.v);
    LAUNCHCHK(ctx);
    g.v_epoch = g.xa_epoch;
    g.post_valid = true;
    return AGP_OK;
  }

  // The Gaussian KL of one latent (KLdivergences.jl:11-18), the part of the ELBO that does not depend on the data -- shared by
  // elbo() and elbo_stream().  enqueue: log-diagonal sum of chol(-2 eta2), tr(K^-1 Sigma), |L^-1 (mu - mu0)|^2 into
  // scal_dev[2..4]; finish: once the caller has read scal_dev[0..4] into h behind a synchronisation, add the latent's KL to *kl.
  agp_status gauss_kl_enqueue(Latent& g, bool use_stale) {
    AGPCHK(materialize(g));
    hipLaunchKernelGGL((k_logdiag_sum<T>), dim3(1), dim3(1024), 0, st(), (const T*)g.DgA, m, scal_dev + 2);
    AGPCHK(frob_dot((const T*)(use_stale ? g.sKinv : g.Kinv), (const T*)g.Sigma, mp, m, scal_dev + 3));
    hipLaunchKernelGGL((k_axpby<T>), grid1(mp), dim3(256), 0, st(), mp, T(1), (const T*)g.mu, T(-1), (const T*)g.mu0,
                       tmpv);
    hipLaunchKernelGGL((k_trmv_lower<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)(use_stale ? g.sXk : g.Xk), mp, mp,
                       (const T*)tmpv, pw0);
    hipLaunchKernelGGL((k_sumsq<T>), dim3(1), dim3(1024), 0, st(), (const T*)pw0, mp, scal_dev + 4);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  agp_status gauss_kl_finish(Latent& g, bool use_stale, const double* h, double* kl) {
    AGPCHK(resolve_logdet(g));
    const double logdetK = 2.0 * (use_stale ? g.s_half_logdetK : g.half_logdetK), logdetS = -2.0 * h[2];
    *kl += 0.5 * (logdetK - logdetS + h[3] + h[4] - (double)m);
    if (g.on) {
      double ek = 0.0;
      AGPCHK(extra_kl(g, &ek));
      *kl += ek;
    }
    return AGP_OK;
  }

  agp_status elbo(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho, int fresh,
                  double* out) override {
    AGPCHK(check_batch(B));
    const bool lsm = lp.kind == AGP_LIK_LOGISTICSOFTMAX;
    const T* mf;
    const T* vf;
    if (mo_sharded) {
      if (fresh || fall_state != 2) {
        ctx->err = "latent-sharded multi-output ELBO: fresh_local = 0 only, after agp_svgp_mo_refresh_f + the all-reduce "
                   "of the exchange buffer";
        return fresh ? AGP_ERR_UNSUPPORTED : AGP_ERR_INVALID;
      }
      if (B != B_last) return AGP_ERR_INVALID;
      mf = fall;
      vf = fall + (int64_t)qtot * Bp;
    } else if (fresh) {
      // ELBO.jl:32-47 : recompute kernel matrices on (x, y), fresh local variables, one local update
      if (lsm) {
        HIPCHK(ctx, hipMemcpyAsync(alpha_save, alpha, sizeof(T) * Bp, hipMemcpyDeviceToDevice, st()));
        hipLaunchKernelGGL((k_fill<T>), grid1(Bp), dim3(256), 0, st(), alpha, Bp, (T)desc.lik.n_class);
      }
      if (mo) HIPCHK(ctx, hipMemcpyAsync(mo_th_save, mo_th, sizeof(T) * MO_MAXT * Bp, hipMemcpyDeviceToDevice, st()));
      // the Gaussian KL below needs Sigma, mu anyway: factor -2*eta2 WITH its inverse first, so that the local step on the
      // evaluation batch (and the next training step) take W, v from the inverse instead of two more factorisation chains
      for (auto& g : lat) AGPCHK(materialize(g));
      eval_cache_ok = true;  // (only this caller: the online model's fresh local steps see new data behind the same pointers)
      const agp_status sl = step_local(x, ldx, y, idx, B, rho, true);
      eval_cache_ok = false;
      AGPCHK(sl);
      if (lsm) {
        for (int it = 0; it < 2; ++it) {
          AGPCHK(lsm_gamma());
          AGPCHK(lsm_alpha());
        }
        AGPCHK(lsm_finish());
      }
      for (auto& g : lat) g.kappa_valid = false;  // (the training step's kappa is gone; the evaluation batch's stays: kappa_eval)
      mf = muf;
      vf = varf;
    } else {
      if (B != B_last) {
        ctx->err = "agp_svgp_elbo(fresh_local=0) must be called with the batch of the last cavi_step";
        return AGP_ERR_INVALID;
      }
      // mean_f / var_f with the UPDATED posterior, local variables from the step (analyticVI.jl:260-266)
      AGPCHK(posterior_f(B));
      mf = emuf;
      vf = evarf;
    }
    if (mo) {
      // multi-output ELBO (analyticVI.jl:277-297): per-task terms on the A-mixed mean_f / var_f
      if (!fresh)
        hipLaunchKernelGGL((k_mo_local<T>), grid1(B), dim3(256), 0, st(), B, Qa(), Bp, mocfg, (const T*)A_dev, (T)rho,
                           (const T*)y, ystride, idx, mf, vf, mo_mixm, mo_mixv, mo_th, mo_cc, rbuf, wbuf, 0, qlo, nl);
      for (int t = 0; t < nT; ++t) {
        LikParams<T> lt{mocfg.kind[t], mocfg.p0[t], mocfg.p1[t]};
        AGPCHK(launch_elbo_terms(B, 1, lt, 0, 0, (const T*)y + t, (const int32_t*)nullptr, idx,
                                 (const T*)(mo_mixm + (int64_t)t * Bp), (const T*)(mo_mixv + (int64_t)t * Bp),
                                 (const T*)(mo_cc + (int64_t)t * Bp), (const T*)(mo_th + (int64_t)t * Bp), (const T*)nullptr,
                                 (const T*)nullptr, (const T*)nullptr, scal_dev + 8 + 2 * t, (int64_t)nT));
      }
      LAUNCHCHK(ctx);
      std::vector<double> ht(2 * nT);
      HIPCHK(ctx, hipMemcpyAsync(ht.data(), scal_dev + 8, sizeof(double) * 2 * nT, hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      mo_e = mo_kl = 0.0;
      for (int t = 0; t < nT; ++t) {
        mo_e += ht[2 * t];
        mo_kl += ht[2 * t + 1];
      }
      if (fresh) HIPCHK(ctx, hipMemcpyAsync(mo_th, mo_th_save, sizeof(T) * MO_MAXT * Bp, hipMemcpyDeviceToDevice, st()));
    } else {
      AGPCHK(launch_elbo_terms(B, nl, lp, desc.latent_offset, (int)(desc.latent_offset == 0), (const T*)y, (const int32_t*)y, idx,
                               (const T*)mf, (const T*)vf, (const T*)cbuf, (const T*)theta, (const T*)gamma, (const T*)alpha,
                               (const T*)beta, scal_dev, (int64_t)1));
    }
    if (fresh && lsm)
      HIPCHK(ctx, hipMemcpyAsync(alpha, alpha_save, sizeof(T) * Bp, hipMemcpyDeviceToDevice, st()));
    // GaussianKL per latent (KLdivergences.jl:11-18)
    double kl_gauss = 0.0;
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      // objective(model, state, y) reads the state's kernel matrices -- the frozen ones under AGP_FLAG_STALE_K; the external
      // ELBO(model, X, y) recomputes them (ELBO.jl:32-47)
      const bool use_stale = g.stale_on && !fresh;
      AGPCHK(gauss_kl_enqueue(g, use_stale));
      if (elbo_async >= 0 && nl == 1 && !mo && !g.on && !use_stale && logdetK_dev) {
        // agp_svgp_elbo_enqueue: the scalar is put together on the device and lands in mapped host memory behind an event
        hipLaunchKernelGGL(k_elbo_combine, dim3(1), dim3(1), 0, st(), (const double*)scal_dev, (const double*)logdetK_dev, (double)m,
                           rho, elbo_pin + elbo_async);
        LAUNCHCHK(ctx);
        HIPCHK(ctx, hipEventRecord(elbo_ev[elbo_async], st()));
        elbo_async_used = true;
        *out = 0.0;
        return AGP_OK;
      }
      double h[5];
      HIPCHK(ctx, hipMemcpyAsync(h, scal_dev, sizeof(double) * 5, hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      if (l == 0) {
        e_data = mo ? mo_e : h[0];
        kl_aug = mo ? mo_kl : h[1];
      }
      AGPCHK(gauss_kl_finish(g, use_stale, h, &kl_gauss));
    }
    // sharded multi-output: the (replicated) data terms are counted by the rank that owns latent 0, the Gaussian KLs by their
    // owners; the driver sums the scalars over ranks
    if (mo_sharded && qlo != 0) e_data = kl_aug = 0.0;
    kl_gauss_last = kl_gauss;
    *out = rho * e_data - kl_gauss - rho * kl_aug;
    return AGP_OK;
  }
  double e_data = 0, kl_aug = 0, mo_e = 0, mo_kl = 0, kl_gauss_last = 0;
  bool shard_once = true;

  // ---- ELBO without a host round trip (round 4): agp_svgp_elbo_enqueue / agp_svgp_elbo_fetch --------------------------------------
  // Convergence monitoring evaluates the ELBO every few iterations; the synchronous call costs a stream synchronisation and a
  // read-back each time (C2: ~1 ms of idle GPU per check, a fifth of the time to the ELBO plateau).  enqueue() puts the same
  // evaluation into the stream and returns a ticket; the value arrives in mapped host memory behind an event, and fetch() reads it
  // when the caller wants it (wait = 0: only if it is there).  Models whose ELBO needs host-side pieces (several latents,
  // multi-output, streaming prior, the frozen matrices of AGP_FLAG_STALE_K) are evaluated synchronously inside enqueue().
  static constexpr int ELBO_RING = 8;
  double* elbo_pin = nullptr;
  hipEvent_t elbo_ev[ELBO_RING] = {};
  bool elbo_ready[ELBO_RING] = {};   // the value was computed synchronously (elbo_val)
  bool elbo_open[ELBO_RING] = {};
  double elbo_val[ELBO_RING] = {};
  int elbo_next = 0, elbo_async = -1;
  bool elbo_async_used = false;
  agp_status elbo_enqueue(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho, int fresh,
                          int32_t* ticket) override {
    if (!ticket) return AGP_ERR_INVALID;
    if (!elbo_pin) {
      HIPCHK(ctx, hipHostMalloc((void**)&elbo_pin, sizeof(double) * ELBO_RING, hipHostMallocMapped));
      for (auto& e : elbo_ev) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // any closed slot will do (tickets may be fetched out of order), searched from the one after the last ticket handed out
    int slot = -1;
    for (int q = 0; q < ELBO_RING && slot < 0; ++q)
      if (!elbo_open[(elbo_next + q) % ELBO_RING]) slot = (elbo_next + q) % ELBO_RING;
    if (slot < 0) {
      ctx->err = "agp_svgp_elbo_enqueue: 8 evaluations in flight, none fetched (agp_svgp_elbo_fetch closes a ticket)";
      return AGP_ERR_INVALID;
    }
    // a batch-sharded handle's ELBO is a sum over the ranks (agp_svgp_elbo_multi): its local terms are what agp_svgp_elbo_terms
    // reports after a SYNCHRONOUS evaluation -- the enqueued form would leave them stale
    const bool force_sync = bs_world > 1;
    elbo_async = force_sync ? -1 : slot;
    elbo_async_used = false;
    double v = 0.0;
    const agp_status st_ = elbo(x, ldx, y, idx, B, rho, fresh, &v);
    elbo_async = -1;
    AGPCHK(st_);
    if (elbo_async_used && fresh && pf_stream) {
      // The evaluation's local step ran on the CURRENT kernel-matrix buffers (Knm, Wbuf, K~ slices) after its step_local had
      // released them to the look-ahead (a fresh step between two CAVI steps releases the previous step's buffers where it starts).
      // With the synchronous call the host waits for the evaluation before it enqueues anything else; here the look-ahead after
      // next could overwrite them while the evaluation still reads them (seen as ELBO values off by tens of per cent): the release
      // it will wait for is recorded again, behind the evaluation.
      const int sl = step_parity ^ 1;
      slot_kind[sl] = 0;
      HIPCHK(ctx, hipEventRecord(step_done[sl], st()));
    }
    elbo_ready[slot] = !elbo_async_used;
    elbo_val[slot] = v;
    elbo_open[slot] = true;
    elbo_next = (slot + 1) % ELBO_RING;
    *ticket = slot;
    return AGP_OK;
  }
  agp_status elbo_fetch(int32_t ticket, int wait, double* out, int32_t* ready) override {
    if (ticket < 0 || ticket >= ELBO_RING || !elbo_open[ticket] || !out) return AGP_ERR_INVALID;
    if (!elbo_ready[ticket]) {
      if (wait) {
        HIPCHK(ctx, hipEventSynchronize(elbo_ev[ticket]));
      } else {
        const hipError_t q = hipEventQuery(elbo_ev[ticket]);
        if (q == hipErrorNotReady) {
          (void)hipGetLastError();
          if (ready) *ready = 0;
          return AGP_OK;
        }
        HIPCHK(ctx, q);
      }
      elbo_val[ticket] = elbo_pin[ticket];
      elbo_ready[ticket] = true;
    }
    *out = elbo_val[ticket];
    elbo_open[ticket] = false;
    if (ready) *ready = 1;
    return AGP_OK;
  }
  // this handle sees shard bs_rank of bs_world of every minibatch (batch-parallel).  Set by agp_svgp_set_batch_shard and -- so that
  // a host cannot forget it after a handle was re-created -- by every batch-mode *_multi call from its communicator.
  int bs_rank = 0, bs_world = 1;
  void adopt_batch_shard(const agp_comm* cm, int mode) {
    if (mode == AGP_SHARD_BATCH && cm && cm->world > 1) {
      bs_rank = cm->rank;
      bs_world = cm->world;
      shard_once = bs_rank == 0;
    }
  }
  agp_status set_batch_shard(int rank, int world) override {
    if (world < 1 || rank < 0 || rank >= world) return AGP_ERR_INVALID;
    shard_once = rank == 0;
    bs_rank = rank;
    bs_world = world;
    return AGP_OK;
  }
  agp_status elbo_terms(double* out3) override {
    if (!out3) return AGP_ERR_INVALID;
    out3[0] = e_data;
    out3[1] = kl_gauss_last;
    out3[2] = kl_aug;
    return AGP_OK;
  }

  // ---- streamed full-data ELBO (include/agp_hip.h, "STREAMED ELBO") ---------------------------------------
  // ELBO(model, X, y) of ELBO.jl:28-47 over any number of points: the predictor's chunk loop (predict_f_latent) leaves the
  // moments of 4096 points in es_mu / es_var, k_elbo_stream_terms forms the fresh local variables in registers and writes one pair
  // of partial sums per workgroup, k_elbo_stream_reduce adds all of them in a fixed order.  Touches the predictor's workspace and
  // caches (Kstar, ppm, ppv, apred / Apred, Tw2) and buffers of its own -- never the step's batch buffers, local variables, kappa
  // caches, look-ahead, status words or the terms of the last agp_svgp_elbo.
  T *es_mu = nullptr, *es_var = nullptr;  // [nl][4096]
  double* es_part = nullptr;              // [ceil(n / 256)][2]
  int64_t es_part_cap = 0;                // (in workgroups)
  double* es_scal = nullptr;              // out[4] of k_elbo_stream_reduce | the two failure words
  agp_status elbo_stream_check_handle() {
    if (lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_HETEROSCEDASTIC)
      return elbo_stream_refused(lp.kind == AGP_LIK_POISSON
                                     ? "Poisson is not supported (lambda is re-estimated from sums over the whole batch: a second pass)"
                                     : "Heteroscedastic is not supported (lambda is re-estimated from sums over the whole batch: a "
                                       "second pass)");
    if (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev)
      return elbo_stream_refused("Gaussian with opt_noise is not supported (its fresh ELBO steps the noise from sums over the batch)");
    if (desc.lik.kind == AGP_LIK_MULTIOUTPUT || mo)
      return elbo_stream_refused("multi-output handles (AGP_LIK_MULTIOUTPUT) are not supported");
    for (auto& g : lat)
      if (g.on) return elbo_stream_refused("online handles (streaming prior) are not supported");
    if (stale_mode()) return elbo_stream_refused("AGP_FLAG_STALE_K handles are not supported");
    if (desc.latent_offset != 0 || mo_sharded || (lp.kind == AGP_LIK_LOGISTICSOFTMAX && desc.n_latent != desc.lik.n_class))
      return elbo_stream_refused("latent-sharded handles are not supported (the local update needs every latent on one handle)");
    if (bs_world > 1) return elbo_stream_refused("batch-sharded handles are not supported");
    return AGP_OK;
  }
  agp_status elbo_stream(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t n, double rho, double* out,
                         double* terms) override {
    AGPCHK(elbo_stream_check_handle());
    if (n <= 0) {
      ctx->err = "agp_svgp_elbo_stream: the number of points " + std::to_string(n) + " is incorrect (it must be positive)";
      return AGP_ERR_BAD_BATCH;
    }
    if (!x || !y || !out || ldx < D || !(rho > 0.0)) {
      ctx->err = "agp_svgp_elbo_stream: x, y and elbo_host must not be NULL, ldx >= D, rho > 0";
      return AGP_ERR_INVALID;
    }
    const int64_t CH = 4096;
    const int64_t nw = (n + ELBO_STREAM_THREADS - 1) / ELBO_STREAM_THREADS;
    for (auto& g : lat) AGPCHK(params_to_host(g));  // k_predict_finish takes the variance by value
    AGPCHK(ensure_pred_ws(0, true));
    if (!es_mu) {
      AGPCHK(dmalloc(ctx, &es_mu, (int64_t)nl * CH));
      AGPCHK(dmalloc(ctx, &es_var, (int64_t)nl * CH));
      AGPCHK(dmalloc(ctx, &es_scal, 8));
    }
    if (nw > es_part_cap) {
      if (es_part) dfree(es_part);
      es_part = nullptr;
      es_part_cap = 0;
      AGPCHK(dmalloc(ctx, &es_part, 2 * nw));
      es_part_cap = nw;
    }
    for (auto& g : lat) {
      AGPCHK(ensure_pred(g, true));
      AGPCHK(ensure_zsc(g));
    }
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(es_scal + 4);
    HIPCHK(ctx, hipMemsetAsync(bad, 0xFF, 2 * sizeof(unsigned long long), st()));
    const bool lsm = lp.kind == AGP_LIK_LOGISTICSOFTMAX;
    for (int64_t s = 0; s < n; s += CH) {
      const int64_t nc = (n - s) < CH ? (n - s) : CH;
      const int64_t nq = rup64(nc);
      // the gather goes through the kernel-matrix kernel: with idx the chunk is idx[s .. s + nc) into the whole x
      const T* xs = idx ? (const T*)x : (const T*)x + s * ldx;
      const int64_t* is = idx ? idx + s : nullptr;
      for (int l = 0; l < nl; ++l) {
        Latent& g = lat[l];
        const int slices = launch_kernelmatrix<T>(ctx, st(), xs, ldx, is, nc, (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind,
                                                  kvar(g), Kstar, mp, nq, mp, 0, T(0), (const T*)g.apred, ppm, CH, 0,
                                                  (const T*)g.Zsc, (const T*)g.zn);
        LAUNCHCHK(ctx);
        AGPCHK((gemm_nt<T, EPI_ROWDOT>(ctx, Kstar, mp, g.Apred, mp, nq, mp, mp, 0, nullptr, 0, Kstar, mp, nullptr, ppv, nullptr,
                                       CH)));
        hipLaunchKernelGGL((k_predict_finish<T>), grid1(nc), dim3(256), 0, st(), nc, slices, (const T*)ppm, (int)(2 * mp / TILE),
                           (const T*)ppv, CH, (T)g.k.variance, (T)jitter, es_mu + (int64_t)l * CH, es_var + (int64_t)l * CH);
        LAUNCHCHK(ctx);
      }
      const unsigned gw = (unsigned)((nc + ELBO_STREAM_THREADS - 1) / ELBO_STREAM_THREADS);
      double* part = es_part + 2 * (s / ELBO_STREAM_THREADS);
#define AGP_ELBO_STREAM_CASE(K)                                                                                                  \
  case K:                                                                                                                        \
    hipLaunchKernelGGL((k_elbo_stream_terms<T, K>), dim3(gw), dim3(ELBO_STREAM_THREADS), 0, st(), nc, s, nl, CH, lp,              \
                       (int)desc.elbo_mode, (const T*)y, (const int32_t*)y, idx, (const T*)es_mu, (const T*)es_var,              \
                       (int)desc.lik.n_class, part, bad);                                                                       \
    break;
      switch (lp.kind) {
        AGP_ELBO_STREAM_CASE(LIK_GAUSSIAN)
        AGP_ELBO_STREAM_CASE(LIK_LOGISTIC)
        AGP_ELBO_STREAM_CASE(LIK_STUDENTT)
        AGP_ELBO_STREAM_CASE(LIK_LSM)
        AGP_ELBO_STREAM_CASE(LIK_LAPLACE)
        AGP_ELBO_STREAM_CASE(LIK_BSVM)
        AGP_ELBO_STREAM_CASE(LIK_NEGBIN)
        default:
          return elbo_stream_refused("unknown likelihood kind");
      }
#undef AGP_ELBO_STREAM_CASE
      LAUNCHCHK(ctx);
    }
    // LogisticSoftMax sum(log, first(beta)) (logisticsoftmax.jl:138): once per evaluation; beta = n_class for fresh local variables
    const double once_add = lsm ? std::log((double)(T)desc.lik.n_class) : 0.0;
    hipLaunchKernelGGL(k_elbo_stream_reduce, dim3(1), dim3(1024), 0, st(), (const double*)es_part, nw, once_add,
                       (const unsigned long long*)bad, es_scal);
    LAUNCHCHK(ctx);
    // Gaussian KL per latent; the data terms and the failure words come back with the first latent's scalars (one
    // synchronisation per latent: one for every likelihood but LogisticSoftMax)
    double hs[4] = {0.0, 0.0, -1.0, -1.0}, kl_gauss = 0.0;
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      AGPCHK(gauss_kl_enqueue(g, false));
      double h[5];
      HIPCHK(ctx, hipMemcpyAsync(h, scal_dev, sizeof(double) * 5, hipMemcpyDeviceToHost, st()));
      if (l == 0) HIPCHK(ctx, hipMemcpyAsync(hs, es_scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      if (l == 0) {
        if (hs[2] >= 0.0) {
          ctx->err = "agp_svgp_elbo_stream: var_f is not positive (or a moment is not finite) at point " +
                     std::to_string((int64_t)hs[2]) + " of the stream (K~ has negative values)";
          return AGP_ERR_NEG_KTILDE;
        }
        if (hs[3] >= 0.0) {
          ctx->err = "agp_svgp_elbo_stream: class index outside the likelihood's classes at point " +
                     std::to_string((int64_t)hs[3]) + " of the stream";
          return AGP_ERR_LABELS;
        }
      }
      AGPCHK(gauss_kl_finish(g, false, h, &kl_gauss));
    }
    *out = rho * hs[0] - kl_gauss - rho * hs[1];
    if (terms) {
      terms[0] = hs[0];
      terms[1] = kl_gauss;
      terms[2] = hs[1];
    }
    return AGP_OK;
  }

  agp_status get_state(int l, void* mu, void* sigma, void* eta1, void* eta2) override {
    if (l < 0 || l >= nl) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    if (mu || sigma) AGPCHK(materialize(g));
    if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, g.mu, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    if (eta1) HIPCHK(ctx, hipMemcpyAsync(eta1, g.eta1, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    if (sigma)
      HIPCHK(ctx, hipMemcpy2DAsync(sigma, sizeof(T) * m, g.Sigma, sizeof(T) * mp, sizeof(T) * m, m,
                                   hipMemcpyDeviceToDevice, st()));
    if (eta2)
      HIPCHK(ctx, hipMemcpy2DAsync(eta2, sizeof(T) * m, g.eta2, sizeof(T) * mp, sizeof(T) * m, m,
                                   hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }

  agp_status set_state(int l, const void* eta1, const void* eta2) override {
    if (l < 0 || l >= nl || !eta1 || !eta2) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    HIPCHK(ctx, hipMemsetAsync(g.eta1, 0, sizeof(T) * mp, st()));
    HIPCHK(ctx, hipMemcpyAsync(g.eta1, eta1, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)eta2, m, m, m, g.eta2, mp, mp, mp,
                       T(-0.5), T(1));
    hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)eta2, m, m, m, g.La, mp, mp, mp, T(1),
                       T(-2));
    LAUNCHCHK(ctx);
    return refactor(g);
  }

  int64_t last_batch() override { return B_last; }
  // init_state(model) (src/training/states.jl:1-9), what train! does when called without a state: fresh local variables
  // (LogisticSoftMax alpha = K, states.jl:11-31 -> logisticsoftmax.jl:43-53), RobbinsMonro counters back to 1 (states.jl:61-84,
  // optimisers.jl:12) and new hyper-optimiser states.  The posterior (eta1, eta2) belongs to the model, not the state: kept.
  agp_status init_state() override {
    n_opt = 1;
    if (noise_adam) HIPCHK(ctx, hipMemsetAsync(noise_adam, 0, sizeof(double) * 6, st()));  // init_local_vars: new state_sigma2
    const T kk = (T)(lp.kind == AGP_LIK_LOGISTICSOFTMAX ? desc.lik.n_class : 1);
    hipLaunchKernelGGL((k_fill<T>), grid1(Bp), dim3(256), 0, st(), alpha, Bp, kk);
    LAUNCHCHK(ctx);
    for (auto& g : lat) {
      g.k_m.clear();
      g.k_v.clear();
      g.k_step = 0;
      g.z_step = 0;
      if (g.kadam) HIPCHK(ctx, hipMemsetAsync(g.kadam, 0, sizeof(double) * 2 * (1 + D), st()));
      if (g.z_am) {
        HIPCHK(ctx, hipMemsetAsync(g.z_am, 0, sizeof(double) * m * D, st()));
        HIPCHK(ctx, hipMemsetAsync(g.z_av, 0, sizeof(double) * m * D, st()));
      }
    }
    return invalidate_data();
  }
  // the caller refilled / mutated X (or y) in place: nothing cached from it may be reused (AnalyticVI kappa cache, look-ahead)
  agp_status invalidate_data() override {
    for (auto& g : lat) g.kappa_valid = g.kappa_eval = false;
    pf_valid = false;
    x_last = nullptr;
    idx_last = nullptr;
    return AGP_OK;
  }

  agp_status get_matrix(int l, int which, void* out, int64_t ldo, int64_t cap) override {
    if (mo && (which == AGP_VEC_THETA || which == AGP_VEC_C)) {
      // multi-output (MOSVGP, MOVGP): the local variables belong to the task likelihoods, `l` counts the tasks
      if (l < 0 || l >= nT || !out || B_last <= 0 || cap < B_last) return AGP_ERR_INVALID;
      HIPCHK(ctx, hipMemcpyAsync(out, (which == AGP_VEC_THETA ? mo_th : mo_cc) + (int64_t)l * Bp, sizeof(T) * B_last,
                                 hipMemcpyDeviceToDevice, st()));
      return AGP_OK;
    }
    if (l < 0 || l >= nl || !out || cap <= 0) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    const int64_t B = B_last;
    const bool m_sized = which == AGP_MAT_L || which == AGP_MAT_KINV;
    if (m_sized ? cap < m : (which != AGP_VEC_ALPHA && (B <= 0 || cap < B))) {
      ctx->err = "agp_svgp_get_matrix: output capacity " + std::to_string(cap) + " is smaller than what the last batch left (" +
                 std::to_string(m_sized ? m : B) + ")";
      return AGP_ERR_INVALID;
    }
    auto copy2 = [&](const T* src, int64_t lds, int64_t rows, int64_t cols) -> agp_status {
      if (ldo < cols) return AGP_ERR_INVALID;
      HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(T) * ldo, src, sizeof(T) * lds, sizeof(T) * cols, rows,
                                   hipMemcpyDeviceToDevice, st()));
      return AGP_OK;
    };
    auto copy1 = [&](const T* src, int64_t n) -> agp_status {
      HIPCHK(ctx, hipMemcpyAsync(out, src, sizeof(T) * n, hipMemcpyDeviceToDevice, st()));
      return AGP_OK;
    };
    switch (which) {
      case AGP_MAT_L: {
        AGPCHK(refresh_K());
        hipLaunchKernelGGL((k_publish_diag<T>), dim3((unsigned)(mp / TILE)), dim3(256), 0, st(), g.L, mp, (const T*)g.DgK);
        LAUNCHCHK(ctx);
        AGPCHK(copy2(g.L, mp, m, m));
        // strict upper part of the stored factor is not maintained outside the diagonal tiles: zero it in the copy
        hipLaunchKernelGGL((k_zero_strict_upper<T>), grid2(m, m), blk2, 0, st(), (T*)out, ldo, m);
        LAUNCHCHK(ctx);
        return AGP_OK;
      }
      case AGP_MAT_KINV:
        AGPCHK(refresh_K());
        return copy2(g.Kinv, mp, m, m);
      case AGP_MAT_KNM:
        return copy2(g.Knm, mp, B, m);
      case AGP_MAT_KAPPA:
        return copy2(g.kappa, mp, B, m);
      case AGP_VEC_KTILDE:
        return copy1(Kt + l * Bp, B);
      case AGP_VEC_MEAN_F:
        return copy1(muf + l * Bp, B);
      case AGP_VEC_VAR_F:
        return copy1(varf + l * Bp, B);
      case AGP_VEC_THETA:
        return copy1(theta + l * Bp, B);
      case AGP_VEC_C:
        return copy1(cbuf + l * Bp, B);
      case AGP_VEC_GAMMA:
        return copy1(gamma + l * Bp, B);
      case AGP_VEC_ALPHA:  // state carried across minibatches: exported by capacity, not by the last batch
        return copy1(alpha, std::min<int64_t>(cap, Bmax));
      default:
        return AGP_ERR_INVALID;
    }
  }

  // ---- prediction (predictions.jl:25-50) -------------------------------------------------------------------
  virtual agp_status ensure_pred(Latent& g, bool need_var) {
    AGPCHK(refresh_K());
    AGPCHK(materialize(g));
    if (!g.apred) {
      AGPCHK(dmalloc(ctx, &g.apred, mp));
    }
    if (need_var && !g.Apred) AGPCHK(dmalloc(ctx, &g.Apred, mp * mp));
    if (!g.pred_valid) {
      // K \ mu
      hipLaunchKernelGGL((k_symv<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Kinv, mp, mp, (const T*)g.mu,
                         g.apred);
      LAUNCHCHK(ctx);
      g.pred_valid = true;
    }
    if (need_var && !g.predvar_valid) {
      // A = K \ (I - Sigma / K) = Kinv - Kinv Sigma Kinv :  T2 = Kinv Sigma (NT, both symmetric) ; A = Kinv - Kinv T2'
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Kinv, mp, g.Sigma, mp, mp, mp, mp, 0, Tw2, mp, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0)));
      tw2_kis_of = (int)(&g - lat.data());  // the hyper-gradient reuses K^-1 Sigma (hypergrad, one_product)
      {  // (symmetric result: lower tiles only, mirrored -- half the flops of the full EPI_EMINUS product)
        const int64_t ntm = mp / TILE, tiles = ntm * (ntm + 1) / 2;
        if (tiles <= 160 && mp >= 8 * BK)  // fewer tiles than CUs: four k-groups per workgroup, like the symmetric product (syrk_tn)
          hipLaunchKernelGGL((k_gemm_nt_eminus_sym<T, 4>), dim3((unsigned)tiles), dim3(4 * NTHREADS), 0, st(), (const T*)g.Kinv, mp,
                             (const T*)Tw2, mp, mp, g.Apred, mp, (const T*)g.Kinv, mp);
        else if (tiles <= kg2_limit() && mp >= 4 * BK)
          hipLaunchKernelGGL((k_gemm_nt_eminus_sym<T, 2>), dim3((unsigned)tiles), dim3(2 * NTHREADS), 0, st(), (const T*)g.Kinv, mp,
                             (const T*)Tw2, mp, mp, g.Apred, mp, (const T*)g.Kinv, mp);
        else
          hipLaunchKernelGGL((k_gemm_nt_eminus_sym<T, 1>), dim3((unsigned)tiles), dim3(NTHREADS), 0, st(), (const T*)g.Kinv, mp,
                             (const T*)Tw2, mp, mp, g.Apred, mp, (const T*)g.Kinv, mp);
        LAUNCHCHK(ctx);
      }
      g.predvar_valid = true;
    }
    return AGP_OK;
  }

  agp_status ensure_pred_ws(int64_t nt, bool need_var) {
    const int64_t CH = 4096;
    if (pred_chunk == 0) {
      pred_chunk = CH;
      AGPCHK(dmalloc(ctx, &ppm, (mp / TILE) * CH));
      AGPCHK(dmalloc(ctx, &ppv, (2 * mp / TILE) * CH));
    }
    if (need_var && !Kstar) AGPCHK(dmalloc(ctx, &Kstar, CH * mp));
    if (nt > pred_nt_cap) {
      if (pmu) (void)hipFree(pmu);
      if (pvar) (void)hipFree(pvar);
      AGPCHK(dmalloc(ctx, &pmu, nl * nt));
      AGPCHK(dmalloc(ctx, &pvar, nl * nt));
      pred_nt_cap = nt;
    }
    return AGP_OK;
  }

  // multi-output: latent predictions mixed by A (predictions.jl:52-92) -> T[n_task][n_t]
  agp_status predict_f(const void* xt, int64_t ldx, int64_t nt, void* mu_out, void* var_out) override {
    if (!mo) return predict_f_latent(xt, ldx, nt, mu_out, var_out);
    AGPCHK(ensure_pred_ws(nt, var_out != nullptr));
    if (nt > mo_pred_cap) {
      if (mo_pmu) (void)hipFree(mo_pmu);
      if (mo_pvar) (void)hipFree(mo_pvar);
      AGPCHK(dmalloc(ctx, &mo_pmu, (int64_t)nl * nt));
      AGPCHK(dmalloc(ctx, &mo_pvar, (int64_t)nl * nt));
      mo_pred_cap = nt;
    }
    AGPCHK(predict_f_latent(xt, ldx, nt, mo_pmu, var_out ? mo_pvar : nullptr));
    // a latent-sharded handle returns its PARTIAL mix (own columns of A): summed over ranks it is the full one
    hipLaunchKernelGGL((k_mo_mix<T>), grid1(nt), dim3(256), 0, st(), nt, nl, nT, (const T*)(A_dev + qlo), Qa(),
                       (const T*)mo_pmu, nt, (T*)mu_out, nt, 0);
    if (var_out)
      hipLaunchKernelGGL((k_mo_mix<T>), grid1(nt), dim3(256), 0, st(), nt, nl, nT, (const T*)(A_dev + qlo), Qa(),
                         (const T*)mo_pvar, nt, (T*)var_out, nt, 1);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  T *mo_pmu = nullptr, *mo_pvar = nullptr;
  int64_t mo_pred_cap = 0;

  agp_status predict_f_latent(const void* xt, int64_t ldx, int64_t nt, void* mu_out, void* var_out) {
    if (!xt || nt <= 0 || ldx < D || !mu_out) return AGP_ERR_INVALID;
    for (auto& g : lat) AGPCHK(params_to_host(g));  // k_predict_finish takes the variance by value
    const bool need_var = var_out != nullptr;
    AGPCHK(ensure_pred_ws(0, need_var));
    for (auto& g : lat) {
      AGPCHK(ensure_pred(g, need_var));
      AGPCHK(ensure_zsc(g));
    }
    const int64_t CH = pred_chunk;
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      if (!need_var && kmm_usable(D)) {
        // means only: ONE launch over all test points, every workgroup carries its 64 rows through all inducing-point tiles with
        // the row-dot against K^-1 mu in registers -- K*m and per-tile partial sums never reach memory (predictions.jl:33-34).
        // (The VALU kernel -- D beyond the MFMA kernel's limit -- leaves one slice per column tile, which the caller's output
        // has no room for: it takes the chunked form below.)
        const int slices = launch_kernelmatrix<T>(ctx, st(), (const T*)xt, ldx, (const int64_t*)nullptr, nt, (const T*)g.Z, D, m, D,
                                                  (const T*)g.scales, g.k.kind, kvar(g), (T*)nullptr, mp, nt, mp, 0, T(0),
                                                  (const T*)g.apred, (T*)mu_out + (int64_t)l * nt, nt, 1, (const T*)g.Zsc,
                                                  (const T*)g.zn);
        LAUNCHCHK(ctx);
        if (slices == 1) continue;
      }
      for (int64_t s = 0; s < nt; s += CH) {
        const int64_t nc = (nt - s) < CH ? (nt - s) : CH;
        const int64_t nq = rup64(nc);
        const T* xs = (const T*)xt + s * ldx;
        const int slices = launch_kernelmatrix<T>(ctx, st(), xs, ldx, (const int64_t*)nullptr, nc, (const T*)g.Z, D, m, D,
                                                  (const T*)g.scales, g.k.kind, kvar(g), need_var ? Kstar : (T*)nullptr, mp,
                                                  nq, mp, 0, T(0), (const T*)g.apred, ppm, CH, 0, (const T*)g.Zsc, (const T*)g.zn);
        LAUNCHCHK(ctx);
        if (need_var)
          AGPCHK((gemm_nt<T, EPI_ROWDOT>(ctx, Kstar, mp, g.Apred, mp, nq, mp, mp, 0, nullptr, 0, Kstar, mp, nullptr, ppv,
                                         nullptr, CH)));
        hipLaunchKernelGGL((k_predict_finish<T>), grid1(nc), dim3(256), 0, st(), nc, slices, (const T*)ppm,
                           (int)(2 * mp / TILE), (const T*)ppv, CH, (T)g.k.variance, (T)jitter,
                           (T*)mu_out + (int64_t)l * nt + s, need_var ? (T*)var_out + (int64_t)l * nt + s : (T*)nullptr);
        LAUNCHCHK(ctx);
      }
    }
    return AGP_OK;
  }

  // ---- input gradients of the predictive moments (include/agp_hip.h, "PREDICTIVE GRADIENTS"; agp_predgrad.h) ----
  // Per chunk of 4096 points and latent: K*m (launch_kernelmatrix) and W = K*m Apred (gemm_nt) when the variances are asked for,
  // then ONE k_predgrad that recomputes the squared distances from x and Z and contracts phi' against the differences, one workgroup
  // per (64 points, group of inducing-point tiles), and k_predgrad_finish, which adds the groups in a fixed order.  A means-only call
  // forms neither K*m nor W.  One routine for every class: it needs only what ensure_pred leaves (apred, Apred).  All buffers are
  // chunk-sized and stay on the handle.
  T* pg_W = nullptr;                     // T[4096][mp]
  double* pg_part = nullptr;             // double[2][PG_MAXGROUPS][4096][D]: the groups' sums of one chunk, mean | variance
  T *pg_gm = nullptr, *pg_gv = nullptr;  // multi-output: the latent gradients of one chunk, T[nl][4096][D]
  agp_status predgrad_refused(const char* why) {
    ctx->err = std::string("agp_svgp_predict_f_grad: ") + why;
    return AGP_ERR_UNSUPPORTED;
  }
  // k_predgrad + k_predgrad_finish of one latent over nc <= 4096 points: gm / gv (nullable) rows pitched by ldo
  template <bool VAR>
  void predgrad_launch(const Latent& g, const T* xs, int64_t ldx, int64_t nc, T* gm, T* gv, int64_t ldo) {
    const int dpt = D <= 4 ? 1 : (D <= 16 ? 4 : (D <= 32 ? 8 : 16));
    const int64_t tpg = pg_tiles_per_group(m, dpt), ntile = (m + pg_ct(dpt) - 1) / pg_ct(dpt), ng = (ntile + tpg - 1) / tpg;
    const dim3 grid((unsigned)((nc + PG_RT - 1) / PG_RT), (unsigned)ng), blk(PG_THREADS);
#define AGP_PG_LAUNCH(DPT)                                                                                                      \
  hipLaunchKernelGGL((k_predgrad<T, DPT, VAR>), grid, blk, 0, st(), xs, ldx, nc, (const T*)g.Z, D, m, (int)D, (const T*)g.scales, \
                     g.k.kind, kvar(g), (const T*)g.apred, (const T*)pg_W, mp, tpg, pg_part)
    if (dpt == 1) AGP_PG_LAUNCH(1);
    else if (dpt == 4) AGP_PG_LAUNCH(4);
    else if (dpt == 8) AGP_PG_LAUNCH(8);
    else AGP_PG_LAUNCH(16);
#undef AGP_PG_LAUNCH
    hipLaunchKernelGGL((k_predgrad_finish<T>), grid1(nc * D), dim3(256), 0, st(), nc, (int)D, (int)ng, (const double*)pg_part,
                       (const T*)g.scales, gm, gv, ldo);
  }
  agp_status predict_f_grad(const void* xt, int64_t ldx, int64_t nt, void* dmu_out, void* dvar_out, int64_t ldg) override {
    if (desc.flags & AGP_FLAG_SAMPLED)
      return predgrad_refused("Gibbs-sampled models (AGP_FLAG_SAMPLED) are not supported: they have no predict_f");
    if (desc.latent_offset != 0 || mo_sharded || (lp.kind == AGP_LIK_LOGISTICSOFTMAX && desc.n_latent != desc.lik.n_class))
      return predgrad_refused("latent-sharded handles are not supported");
    if (bs_world > 1) return predgrad_refused("batch-sharded handles are not supported");
    for (auto& g : lat)
      if (g.k.kind == AGP_K_EXPONENTIAL)
        return predgrad_refused("ExponentialKernel is not differentiable at zero distance");
    if (D > PG_MAXD) return predgrad_refused("the input dimension D must be at most 64 (the hyper-gradient's limit)");
    if (nt < 0 || ldx < D || ldg < D || (nt > 0 && (!xt || !dmu_out))) {
      ctx->err = "agp_svgp_predict_f_grad: n_t >= 0, xt and dmu_out must not be NULL, ldx >= D, ldg >= D";
      return AGP_ERR_INVALID;
    }
    if (nt == 0) return AGP_OK;
    const bool need_var = dvar_out != nullptr;
    const int64_t CH = PG_CH;
    for (auto& g : lat) AGPCHK(params_to_host(g));
    if (!pg_part) AGPCHK(dmalloc(ctx, &pg_part, 2 * (int64_t)PG_MAXGROUPS * CH * D));
    if (need_var) {
      AGPCHK(ensure_pred_ws(0, true));
      if (!pg_W) AGPCHK(dmalloc(ctx, &pg_W, CH * mp));
    }
    if (mo) {
      if (!pg_gm) AGPCHK(dmalloc(ctx, &pg_gm, (int64_t)nl * CH * D));
      if (need_var && !pg_gv) AGPCHK(dmalloc(ctx, &pg_gv, (int64_t)nl * CH * D));
    }
    for (auto& g : lat) {
      AGPCHK(ensure_pred(g, need_var));
      if (need_var) AGPCHK(ensure_zsc(g));
    }
    for (int64_t s = 0; s < nt; s += CH) {
      const int64_t nc = (nt - s) < CH ? (nt - s) : CH;
      const int64_t nq = rup64(nc);
      const T* xs = (const T*)xt + s * ldx;
      for (int l = 0; l < nl; ++l) {
        Latent& g = lat[l];
        if (need_var) {
          (void)launch_kernelmatrix<T>(ctx, st(), xs, ldx, (const int64_t*)nullptr, nc, (const T*)g.Z, D, m, D, (const T*)g.scales,
                                       g.k.kind, kvar(g), Kstar, mp, nq, mp, 0, T(0), (const T*)nullptr, (T*)nullptr, 0, 0,
                                       (const T*)g.Zsc, (const T*)g.zn);
          LAUNCHCHK(ctx);
          AGPCHK((gemm_nt<T, EPI_STORE>(ctx, Kstar, mp, g.Apred, mp, nq, mp, mp, 0, pg_W, mp, nullptr, 0, nullptr, nullptr, nullptr,
                                        0)));
        }
        T* gm = mo ? pg_gm + (int64_t)l * CH * D : (T*)dmu_out + ((int64_t)l * nt + s) * ldg;
        T* gv = !need_var ? (T*)nullptr : (mo ? pg_gv + (int64_t)l * CH * D : (T*)dvar_out + ((int64_t)l * nt + s) * ldg);
        if (need_var) predgrad_launch<true>(g, xs, ldx, nc, gm, gv, mo ? D : ldg);
        else predgrad_launch<false>(g, xs, ldx, nc, gm, gv, mo ? D : ldg);
        LAUNCHCHK(ctx);
      }
      if (mo) {  // the mixed outputs, as predict_f returns them (predictions.jl:52-92)
        hipLaunchKernelGGL((k_predgrad_mix<T>), grid1(nc * D), dim3(256), 0, st(), nc, (int)D, nl, nT, (const T*)A_dev, Qa(),
                           (const T*)pg_gm, CH, (T*)dmu_out + s * ldg, ldg, nt * ldg, 0);
        if (need_var)
          hipLaunchKernelGGL((k_predgrad_mix<T>), grid1(nc * D), dim3(256), 0, st(), nc, (int)D, nl, nT, (const T*)A_dev, Qa(),
                             (const T*)pg_gv, CH, (T*)dvar_out + s * ldg, ldg, nt * ldg, 1);
        LAUNCHCHK(ctx);
      }
    }
    return AGP_OK;
  }

  // ---- acquisition functions (include/agp_hip.h, "ACQUISITION FUNCTIONS") ---------------------------------------
  // The drivers (AcqDriver in agp_acq_host.h, AcqJointDriver in agp_acq_joint_host.h) hold the state of the calls and enqueue every
  // launch; they are Float64 code that serves every class, as predict_f_grad does, because they need only what ensure_pred leaves.
  // Here is what needs the model: the refusals by handle, latent and kernel, and the view of one latent's predictor (AcqModel), in
  // which the predictor's workspaces (Kstar, pg_W, pg_part) are those of predict_f_grad.  Nothing of the latent's is written.
  AcqDriver acqd;
  AcqJointDriver acqjd;
  agp_status acq_refused(const char* who, const char* why) {
    ctx->err = std::string(who) + why;
    return AGP_ERR_UNSUPPORTED;
  }
  agp_status acq_check_handle(const char* who) {
    if (!std::is_same<T, double>::value) return acq_refused(who, "AGP_F32 handles are not supported (the acquisition functions are Float64)");
    if (desc.lik.kind == AGP_LIK_MULTIOUTPUT || mo)
      return acq_refused(who, "multi-output handles (MOSVGP, MOVGP) are not supported");
    if (desc.flags & AGP_FLAG_SAMPLED)
      return acq_refused(who, "Gibbs-sampled models (AGP_FLAG_SAMPLED) are not supported: they have no predict_f");
    if (desc.latent_offset != 0 || mo_sharded || (lp.kind == AGP_LIK_LOGISTICSOFTMAX && desc.n_latent != desc.lik.n_class))
      return acq_refused(who, "latent-sharded handles are not supported");
    if (bs_world > 1) return acq_refused(who, "batch-sharded handles are not supported");
    if (D > PG_MAXD) return acq_refused(who, "the input dimension D must be at most 64 (the hyper-gradient's limit)");
    return AGP_OK;
  }
  // desc and latent, then the latent's kernel
  agp_status acq_check_latent(const char* who, int l, const agp_acq_desc* d, AcqParams* p) {
    AGPCHK(acq_check_desc(ctx, who, d, p));
    if (l < 0 || l >= nl) {
      ctx->err = std::string(who) + "latent must lie in [0, n_latent)";
      return AGP_ERR_INVALID;
    }
    if (lat[l].k.kind == AGP_K_EXPONENTIAL) return acq_refused(who, "ExponentialKernel is not differentiable at zero distance");
    return AGP_OK;
  }
  agp_status acq_check(const char* who, int l, const agp_acq_desc* d, AcqParams* p) override {
    AGPCHK(acq_check_handle(who));
    return acq_check_latent(who, l, d, p);
  }
  agp_status acq_prepare(Latent& g, bool ascent) {
    AGPCHK(params_to_host(g));
    AGPCHK(ensure_pred_ws(0, true));
    if (!pg_part) AGPCHK(dmalloc(ctx, &pg_part, 2 * (int64_t)PG_MAXGROUPS * PG_CH * D));
    if (!pg_W) AGPCHK(dmalloc(ctx, &pg_W, (int64_t)PG_CH * mp));
    AGPCHK(acqd.acq.ensure_chunk(ctx, D, ascent));
    AGPCHK(ensure_pred(g, true));
    AGPCHK(ensure_zsc(g));
    return AGP_OK;
  }
  // the view of a prepared latent (T is double: acq_check_handle has refused every other handle)
  AcqModel acq_model(Latent& g) {
    return AcqModel{ctx, D, m, mp, g.k.kind, (double)kvar(g), g.k.variance + jitter, (const double*)g.scales,
                    AcqPred{(const double*)g.Z, (const double*)g.Zsc, (const double*)g.zn, (const double*)g.apred, (const double*)g.Apred, m,
                            mp, mp, (double*)Kstar, (double*)pg_W, nullptr, nullptr, nullptr, nullptr},
                    (double*)pg_part};
  }
  agp_status acq_open(int l, bool ascent, AcqModel* model, AcqDriver** plain, AcqJointDriver** joint) override {
    AGPCHK(acq_prepare(lat[l], ascent));
    *model = acq_model(lat[l]);
    *plain = &acqd;
    if (joint) *joint = &acqjd;
    return AGP_OK;
  }
  // AGP_VEC_APRED / AGP_MAT_APRED of agp_svgp_get_matrix: the two objects of the predictor after ensure_pred, for every class
  agp_status get_predictor(int l, int which, void* out, int64_t ldo, int64_t cap) override {
    if (desc.flags & AGP_FLAG_SAMPLED) {
      ctx->err = "agp_svgp_get_matrix: Gibbs-sampled models (AGP_FLAG_SAMPLED) have no predictor (AGP_VEC_APRED / AGP_MAT_APRED)";
      return AGP_ERR_UNSUPPORTED;
    }
    const bool mat = which == AGP_MAT_APRED;
    if (l < 0 || l >= nl || !out || cap < m || (mat && ldo < m)) {
      ctx->err = "agp_svgp_get_matrix: AGP_VEC_APRED / AGP_MAT_APRED need latent in [0, n_latent), out given, cap >= m and ldo >= m";
      return AGP_ERR_INVALID;
    }
    Latent& g = lat[l];
    AGPCHK(ensure_pred_ws(0, mat));
    AGPCHK(ensure_pred(g, mat));
    if (mat)
      HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(T) * ldo, g.Apred, sizeof(T) * mp, sizeof(T) * m, m, hipMemcpyDeviceToDevice, st()));
    else
      HIPCHK(ctx, hipMemcpyAsync(out, g.apred, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }

  // ---- pathwise sampling (include/agp_hip.h, "PATHWISE SAMPLING") -----------------------------------------------------------
  // the handles a draw is not built for, by name, before anything is touched
  agp_status pathwise_check_handle() {
    if (!std::is_same<T, double>::value) return pathwise_refused("AGP_F32 handles are not supported (the draw is Float64)");
    if (desc.lik.kind == AGP_LIK_MULTIOUTPUT || mo)
      return pathwise_refused("multi-output handles (MOSVGP, MOVGP) are not supported: draw from single-output models");
    if (desc.latent_offset != 0 || mo_sharded || (lp.kind == AGP_LIK_LOGISTICSOFTMAX && desc.n_latent != desc.lik.n_class))
      return pathwise_refused("latent-sharded handles are not supported (a draw needs every latent on one handle)");
    if (bs_world > 1) return pathwise_refused("batch-sharded handles are not supported");
    return AGP_OK;
  }
  agp_status pathwise_draw(int n_features, int n_samples, uint64_t seed, int64_t t, agp_pathwise** out) override {
    AGPCHK(pathwise_check_handle());
    AGPCHK(pw_check_draw(ctx, m, D, n_features, n_samples, t, out));
    if constexpr (std::is_same<T, double>::value) {
      *out = nullptr;
      AGPCHK(flush());
      AGPCHK(refresh_K());
      std::unique_ptr<agp_pathwise> p;
      AGPCHK(pw_create(ctx, nl, m, D, n_features, n_samples, &p));
      for (int l = 0; l < nl; ++l) {
        Latent& g = lat[l];
        AGPCHK(params_to_host(g));
        AGPCHK(pw_add_latent(*p, l, g.k.kind, g.k.variance, g.scales, g.Z, seed, t));
        AGPCHK(pathwise_latent(*p, l));
      }
      HIPCHK(ctx, hipStreamSynchronize(st()));
      *out = p.release();
    }
    return AGP_OK;
  }
  // V of one latent into the right columns of [W' | V']: U = mu 1' + Xa' E with Xa = chol_lower(-2 eta2)^-1 factored here from the
  // exported eta2 (whatever the step left in La / Xa), R = U - Phi(Z) W, V' = R' K^-1
  virtual agp_status pathwise_latent(agp_pathwise& p, int l) {
    if constexpr (std::is_same<T, double>::value) {
      Latent& g = lat[l];
      PwScratch sc;
      double *mu = nullptr, *e2 = nullptr, *A = nullptr, *X = nullptr, *U = nullptr, *PW = nullptr;
      AGPCHK(sc.get(ctx, &mu, m));
      AGPCHK(sc.get(ctx, &e2, m * m));
      AGPCHK(sc.get(ctx, &A, mp * mp));
      AGPCHK(sc.get(ctx, &X, mp * mp));
      AGPCHK(sc.get(ctx, &U, mp * p.Sp));
      AGPCHK(sc.get(ctx, &PW, mp * p.Sp));
      AGPCHK(get_state(l, mu, nullptr, nullptr, e2));
      AGPCHK(pw_inverse_factor(ctx, sc, A, e2, m, m, mp, -2.0, X));
      AGPCHK(pw_gemm_tn(ctx, X, mp, p.lat[l].E, p.Sp, mp, p.Sp, mp, U, p.Sp));
      AGPCHK(pw_phi_W(p, l, PW));
      hipLaunchKernelGGL(k_pw_resid, grid2(m, p.S), blk2, 0, st(), m, (int64_t)p.S, p.Sp, (const double*)mu, (const double*)PW, U);
      LAUNCHCHK(ctx);
      AGPCHK(pw_gemm_tn(ctx, U, p.Sp, g.Kinv, mp, p.Sp, mp, mp, p.lat[l].WV + p.Lp, p.ldw));
      HIPCHK(ctx, hipStreamSynchronize(st()));  // the scratch goes out of scope
    }
    return AGP_OK;
  }

  agp_status predict_y(const void* xt, int64_t ldx, int64_t nt, void* out) override {
    if (!out) return AGP_ERR_INVALID;
    if (mo) {  // T[n_task][n_t]: regression tasks -> mean ; Bernoulli tasks -> 1.0 / 0.0 (mu_f > 0)
      if (mo_sharded) return sharded_predict_error();
      AGPCHK(predict_f(xt, ldx, nt, out, nullptr));
      return mo_predict_from_f(nt, 0, out, nullptr, nullptr, nullptr, 0);
    }
    if (lp.kind == AGP_LIK_GAUSSIAN || lp.kind == AGP_LIK_STUDENTT || lp.kind == AGP_LIK_LAPLACE)
      return predict_f(xt, ldx, nt, out, nullptr);
    AGPCHK(ensure_pred_ws(nt, false));
    AGPCHK(predict_f(xt, ldx, nt, pmu, nullptr));
    if (lp.kind == AGP_LIK_HETEROSCEDASTIC) {  // heteroscedastic.jl:137-141 : the mean of the first latent
      HIPCHK(ctx, hipMemcpyAsync(out, pmu, sizeof(T) * nt, hipMemcpyDeviceToDevice, st()));
      return AGP_OK;
    }
    if (lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_NEGBINOMIAL) {
      hipLaunchKernelGGL((k_predict_event<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu,
                         (int)(lp.kind == AGP_LIK_NEGBINOMIAL), desc.lik.p0,
                         lp.kind == AGP_LIK_POISSON ? (const T*)lam_dev : (const T*)nullptr, (T*)out);
      LAUNCHCHK(ctx);
      return AGP_OK;
    }
    hipLaunchKernelGGL((k_predict_label<T>), grid1(nt), dim3(256), 0, st(), nt, nl, nt, desc.latent_offset,
                       (const T*)pmu, (int32_t*)out, (int)(lp.kind == AGP_LIK_LOGISTIC || lp.kind == AGP_LIK_BAYESIANSVM));
    LAUNCHCHK(ctx);
    return AGP_OK;
  }

  agp_status upload_gh(const double* nodes, const double* weights, int nn) {
    if (nn > gh_cap) {
      if (gh_dev) (void)hipFree(gh_dev);
      AGPCHK(dmalloc(ctx, &gh_dev, 2 * nn));
      gh_cap = nn;
    }
    HIPCHK(ctx, hipMemcpyAsync(gh_dev, nodes, sizeof(double) * nn, hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipMemcpyAsync(gh_dev + nn, weights, sizeof(double) * nn, hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    gh_n = nn;
    return AGP_OK;
  }
  agp_status set_quadrature(const double* nodes, const double* weights, int nn) override {
    if (!nodes || !weights || nn <= 0) return AGP_ERR_INVALID;
    return upload_gh(nodes, weights, nn);
  }
  agp_status set_lsm_alpha(const void* a, int64_t n) override {
    if (lp.kind != AGP_LIK_LOGISTICSOFTMAX || !a || n <= 0 || n > Bp) return AGP_ERR_INVALID;
    HIPCHK(ctx, hipMemcpyAsync(alpha, a, sizeof(T) * n, hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }
  const void* lpd_lik_state() override {
    return (lp.kind == AGP_LIK_POISSON || (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev)) ? lam_dev : nullptr;
  }
  bool lpd_batch_sharded() override { return bs_world > 1; }
  agp_status get_lik_param(double* out) override {
    if (!out) return AGP_ERR_INVALID;
    if (lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_HETEROSCEDASTIC || (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev)) {
      T v;
      HIPCHK(ctx, hipMemcpyAsync(&v, lam_dev, sizeof(T), hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      *out = (double)v;
    } else {
      *out = desc.lik.p0;
    }
    return AGP_OK;
  }
  agp_status set_lik_param(double v) override {
    if (!(v > 0) || !(lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_HETEROSCEDASTIC ||
                      (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev)))
      return AGP_ERR_INVALID;
    hipLaunchKernelGGL((k_fill<T>), dim3(1), dim3(64), 0, st(), lam_dev, (int64_t)1, (T)v);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }

  agp_status proba_y(const void* xt, int64_t ldx, int64_t nt, const double* nodes, const double* weights, int nn,
                     void* o0, void* o1) override {
    if (!o0) return AGP_ERR_INVALID;
    AGPCHK(ensure_pred_ws(nt, true));
    if (mo) {  // per task compute_proba on the mixed (mu_f, var_f): out0 / out1 are T[n_task][n_t]
      if (!o1) return AGP_ERR_INVALID;
      if (mo_sharded) return sharded_predict_error();
      AGPCHK(predict_f(xt, ldx, nt, o0, o1));
      return mo_predict_from_f(nt, 1, o0, o1, nodes, weights, nn);
    }
    return proba_y_single(xt, ldx, nt, nodes, weights, nn, o0, o1);
  }

  agp_status sharded_predict_error() {
    ctx->err = "latent-sharded multi-output model: predict_f returns the partial mix; all-reduce it and finish with "
               "agp_svgp_mo_predict_from_f";
    return AGP_ERR_UNSUPPORTED;
  }
  // the likelihood half of predict_y (mode 0: o0 = mixed mean_f, in place) / proba_y (mode 1: o0, o1 = mixed mean_f, var_f, in
  // place) of a multi-output model: what follows the mixing in predictions.jl:178-247
  agp_status mo_predict_from_f(int64_t nt, int mode, void* o0, void* o1, const double* nodes, const double* weights,
                               int nn) override {
    if (!mo || !o0 || nt <= 0 || (mode == 1 && !o1)) return AGP_ERR_INVALID;
    if (mode == 0) {
      for (int t = 0; t < nT; ++t) {
        if (mocfg.kind[t] == AGP_LIK_LOGISTIC || mocfg.kind[t] == AGP_LIK_BAYESIANSVM)
          hipLaunchKernelGGL((k_step01<T>), grid1(nt), dim3(256), 0, st(), (T*)o0 + (int64_t)t * nt, nt);
        else if (mocfg.kind[t] == AGP_LIK_NEGBINOMIAL)
          hipLaunchKernelGGL((k_predict_event<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)o0 + (int64_t)t * nt, 1,
                             (double)mocfg.p0[t], (const T*)nullptr, (T*)o0 + (int64_t)t * nt);
      }
      LAUNCHCHK(ctx);
      return AGP_OK;
    }
    {
      for (int t = 0; t < nT; ++t) {
        T* m0 = (T*)o0 + (int64_t)t * nt;
        T* v0 = (T*)o1 + (int64_t)t * nt;
        if (mocfg.kind[t] == AGP_LIK_GAUSSIAN) {
          hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)m0, (const T*)v0,
                             mocfg.p0[t], 0, m0, v0);
        } else if (mocfg.kind[t] == AGP_LIK_STUDENTT) {
          const double nu = (double)mocfg.p0[t], sg = (double)mocfg.p1[t];
          hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)m0, (const T*)v0,
                             (T)(nu * sg * sg / (2.0 * (nu / 2.0 - 1.0))), 1, m0, v0);
        } else if (mocfg.kind[t] == AGP_LIK_LAPLACE) {
          hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)m0, (const T*)v0,
                             (T)(2.0 * (double)mocfg.p0[t] * (double)mocfg.p0[t]), 1, m0, v0);
        } else {
          if (!nodes || !weights || nn <= 0) return AGP_ERR_INVALID;
          if (gh_n != nn) AGPCHK(upload_gh(nodes, weights, nn));
          if (mocfg.kind[t] == AGP_LIK_LOGISTIC)
            hipLaunchKernelGGL((k_proba_logistic<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)m0, (const T*)v0, nn,
                               (const double*)gh_dev, (const double*)(gh_dev + nn), m0, v0);
          else
            hipLaunchKernelGGL((k_proba_gh<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)m0, (const T*)v0, nn,
                               (const double*)gh_dev, (const double*)(gh_dev + nn),
                               mocfg.kind[t] == AGP_LIK_BAYESIANSVM ? 1 : 3, (double)mocfg.p0[t], (const T*)nullptr, m0,
                               v0);
        }
      }
      LAUNCHCHK(ctx);
      return AGP_OK;
    }
  }


  // ---- full predictive covariance (predict_f(...; cov=true, diag=false), predictions.jl:45-49) ------------------------
  //   cov = K** + jitt I - K*m (K^-1 - K^-1 Sigma K^-1) Km*      (K*m materialised: meant for small n_t)
  agp_status predict_f_cov(const void* xt, int64_t ldx, int64_t nt, void* mu_out, void* cov_out) override {
    if (!xt || nt <= 0 || nt > 8192 || ldx < D || !mu_out || !cov_out) return AGP_ERR_INVALID;
    if (mo_sharded) {
      ctx->err = "full predictive covariance of a latent-sharded multi-output model is not wired (partial mixes would have to be "
                 "all-reduced)";
      return AGP_ERR_UNSUPPORTED;
    }
    // multi-output (predictions.jl:52-92): mu_out T[n_task][n_t] = sum_q A[t][q] mu_q, cov_out T[n_task][n_t][n_t] = sum_q A[t][q]^2 Cov_q
    if (mo) AGPCHK(predict_f(xt, ldx, nt, mu_out, nullptr));
    else AGPCHK(predict_f_latent(xt, ldx, nt, mu_out, nullptr));
    const int64_t nq = rup64(nt);
    T *Ks = nullptr, *T1 = nullptr, *Kss = nullptr, *Cq = nullptr;
    AGPCHK(dmalloc(ctx, &Ks, nq * mp));
    AGPCHK(dmalloc(ctx, &T1, nq * mp));
    AGPCHK(dmalloc(ctx, &Kss, nq * nq));
    AGPCHK(dmalloc(ctx, &Cq, nq * nq));
    agp_status rc = AGP_OK;
    for (int l = 0; l < nl && rc == AGP_OK; ++l) {
      Latent& g = lat[l];
      rc = ensure_pred(g, true);
      if (rc != AGP_OK) break;
      dim3 gk((unsigned)(mp / TILE), (unsigned)(nq / TILE));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)xt, ldx, (const int64_t*)nullptr, nt,
                         (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), Ks, mp, nq, mp, 0, T(0),
                         (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
      dim3 gs((unsigned)(nq / TILE), (unsigned)(nq / TILE));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)xt, ldx, (const int64_t*)nullptr, nt,
                         (const T*)xt, ldx, nt, D, (const T*)g.scales, g.k.kind, kvar(g), Kss, nq, nq, nq, 1,
                         (T)jitter, (const T*)nullptr, (T*)nullptr, (int64_t)0);
      rc = gemm_nt<T, EPI_STORE>(ctx, Ks, mp, g.Apred, mp, nq, mp, mp, 0, T1, mp, nullptr, 0, nullptr, nullptr, nullptr, 0);
      if (rc != AGP_OK) break;
      rc = gemm_nt<T, EPI_EMINUS>(ctx, T1, mp, Ks, mp, nq, nq, mp, 0, Cq, nq, Kss, nq, nullptr, nullptr, nullptr, 0);
      if (rc != AGP_OK) break;
      if (mo) {
        hipLaunchKernelGGL((k_mo_cov_acc<T>), grid2(nt, nt), blk2, 0, st(), nt, nT, (const T*)(A_dev + l), (int64_t)Qa(),
                           (const T*)Cq, nq, (T*)cov_out, l == 0 ? 1 : 0);
      } else if (hipMemcpy2DAsync((T*)cov_out + (int64_t)l * nt * nt, sizeof(T) * nt, Cq, sizeof(T) * nq, sizeof(T) * nt, nt,
                                  hipMemcpyDeviceToDevice, st()) != hipSuccess)
        rc = AGP_ERR_HIP;
    }
    (void)hipStreamSynchronize(st());
    dfree(Ks);
    dfree(T1);
    dfree(Kss);
    dfree(Cq);
    return rc;
  }

  // ---- multi-GPU drivers behind the ABI (include/agp_hip.h "multi-GPU") -----------------------
  agp_status comm_sum(agp_comm* cm, void* buf, int64_t count) {
    return comm_sum_typed(cm, buf, count, sizeof(T) == 8 ? AGP_F64 : AGP_F32, force_split());
  }
  // AGP_FORCE_SPLIT=1 (diagnostic): take the phase-split batch-parallel path (statistics -> all-reduce -> eta step) with a one-rank
  // communicator too, and issue its collective, so that its cost next to the fused step can be measured on a single GPU
  static bool force_split() {
    static const bool on = []() {
      const char* e = getenv("AGP_FORCE_SPLIT");
      return e && e[0] == '1';
    }();
    return on;
  }
  agp_status comm_sum_typed(agp_comm* cm, void* buf, int64_t count, int dtype, bool force = false) {
    // (AGP_ALLOW_PARTIAL_SHARD=1: bench.py times ONE rank's share of the 16-latent model on a one-GPU box -- the other latents'
    //  rows of the exchange buffer stay zero, the numbers are meaningless, the work per rank is what is measured)
    static const bool allow_partial = []() {
      const char* e = getenv("AGP_ALLOW_PARTIAL_SHARD");
      return e && e[0] == '1';
    }();
    if (!cm && mo_sharded && nl != qtot && !allow_partial) {
      // a handle that owns a slice of the latents cannot finish a mix, an ELBO or a prediction on its own
      ctx->err = "latent-sharded multi-output handle: this call needs the communicator of the run (comm = NULL)";
      return AGP_ERR_INVALID;
    }
    if (!cm || (cm->world <= 1 && !force)) return AGP_OK;
    if (cm->ctx != ctx) {
      ctx->err = "agp_comm belongs to another ctx (its collectives would run on another stream)";
      return AGP_ERR_INVALID;
    }
    return agp_comm_allreduce(cm, buf, count, dtype);
  }

  // block-column groups of the packed statistics for AGP_SPLIT_OVERLAP: four groups of about equal tile count (8 groups with a
  // 112 us train measured the same step time); group 0 also carries t (it sits in front of block column 0 in `stats`)
  agp_status overlap_groups() {
    const int64_t nt = mp / TILE;
    const int want = (int)std::max<int64_t>(1, std::min<int64_t>(4, nt));
    if (!arrive_dev) {
      HIPCHK(ctx, hipMalloc((void**)&arrive_dev, 8 * ARRIVE_STRIDE * sizeof(int32_t)));
      HIPCHK(ctx, hipMemsetAsync(arrive_dev, 0, 8 * ARRIVE_STRIDE * sizeof(int32_t), st()));
    }
    if (ov_nt == nt && ov_ng == want) return AGP_OK;
    auto cum = [&](int64_t c) { return c * nt - c * (c - 1) / 2; };  // tiles of block columns [0, c)
    const int64_t total = cum(nt);
    int64_t bnd[9];
    bnd[0] = 0;
    for (int g = 1; g < want; ++g) {
      const double tgt = (double)total * g / want;
      int64_t c = bnd[g - 1] + 1;
      while (c < nt - (want - g) && std::fabs((double)cum(c + 1) - tgt) < std::fabs((double)cum(c) - tgt)) ++c;
      bnd[g] = c;
    }
    bnd[want] = nt;
    for (int g = 0; g < want; ++g) {
      ov_off[g] = g == 0 ? 0 : mp + cum(bnd[g]) * TILE * TILE;
      ov_cnt[g] = (g == 0 ? mp : 0) + (cum(bnd[g + 1]) - cum(bnd[g])) * TILE * TILE;
      for (int64_t c = bnd[g]; c < bnd[g + 1]; ++c) ov_grp[c] = (unsigned char)g;
    }
    ov_ng = want;
    ov_nt = nt;
    return AGP_OK;
  }

  agp_status cavi_step_multi(agp_comm* cm, int mode, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                             double rho) override {
    if (mode != AGP_SHARD_LATENT && mode != AGP_SHARD_BATCH) return AGP_ERR_INVALID;
    const bool multi = cm && (cm->world > 1 || (force_split() && mode == AGP_SHARD_BATCH));
    adopt_batch_shard(cm, mode);
    const bool lam_lik = lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_HETEROSCEDASTIC ||
                         (lp.kind == AGP_LIK_GAUSSIAN && lp.noise_dev);  // likelihood state re-estimated from whole-minibatch sums
    if (multi && lam_lik && mode == AGP_SHARD_LATENT) {
      // a Poisson model has one latent, and the two heteroscedastic latents are coupled point-wise and stay on one handle:
      // these models shard over the minibatch only
      ctx->err = "Poisson / Heteroscedastic likelihoods shard over the minibatch (AGP_SHARD_BATCH), not over latents";
      return AGP_ERR_UNSUPPORTED;
    }
    if (mode == AGP_SHARD_BATCH && mo_sharded) return AGP_ERR_INVALID;
    // batch-sharded Poisson / Heteroscedastic: lambda is re-estimated from sums over the WHOLE minibatch (poisson.jl:78,
    // heteroscedastic.jl:94): the local update stops after its partial sums, three doubles are all-reduced, then it finishes
    lam_deferred = multi && lam_lik;
    // batch-parallel over several ranks, one latent: the step rides on the task-graph launches like the one-GPU step does (round 3)
    // -- row statistics as the epilogue of this launch, the eta step from the REDUCED statistics as the prologue of the next one
    // (PendingPacked) -- so that between two factorisations only the packed product, the all-reduce and one 5 us kernel remain.
    // AGP_SPLIT_MERGED=0 keeps the separate kernels (k_safe_rowstats, k_eta2_from_packed).
    static const bool split_merged = []() {
      const char* e = getenv("AGP_SPLIT_MERGED");
      return !(e && e[0] == '0');
    }();
    const bool merge = split_merged && multi && mode == AGP_SHARD_BATCH && !lam_lik && nl == 1 && pro_allowed() &&
                       chol_use_dag(ctx, mp / TILE, rup64(B) / TILE + 1, 1);
    in_cavi_step = merge;
    const agp_status sl = step_local(x, ldx, y, idx, B, rho, false);
    in_cavi_step = false;
    lam_deferred = false;
    AGPCHK(sl);
    AGPCHK(run_deferred_safe());  // (the launch's fallback: the packed product below needs this step's r, w now)
    if (multi && lam_lik) {
      AGPCHK(comm_sum_typed(cm, scal_dev + 60, 3, AGP_F64, force_split()));
      AGPCHK(lambda_finish_reduced());
    }
    const bool lsm = lp.kind == AGP_LIK_LOGISTICSOFTMAX;
    if (mode == AGP_SHARD_LATENT) {
      if (lsm) {
        for (int it = 0; it < 2; ++it) {  // the (gamma, alpha) fixed point needs sum_k gamma_k over ALL latents
          AGPCHK(lsm_gamma());
          AGPCHK(comm_sum(cm, gsum, B_last));
          AGPCHK(lsm_alpha());
        }
      }
      if (mo_sharded) {
        AGPCHK(comm_sum(cm, fall, (int64_t)2 * qtot * Bp));
        AGPCHK(mo_mix());
      }
      AGPCHK(step_stats(true));  // each latent is whole on its rank: the fused natural-gradient step applies
      return step_global(true);
    }
    if (lsm) AGPCHK(lsm_local_all());  // all latents are local: the fixed point is per point, nothing to exchange
    if (!multi) {
      AGPCHK(step_stats(true));
      return step_global(true);
    }
    AGPCHK(step_stats(false));
    // AGP_SPLIT_OVERLAP=1 (default off; read at every call so that bench.py can A/B it in one process): the statistics travel in
    // block-column groups on the communicator's own stream and the next task-graph launch starts on the first group
    // (comm_allreduce_groups).  Only where the step rides on the task-graph launches (`merge`).
    bool overlap = false;
    if (merge) {
      const char* e = getenv("AGP_SPLIT_OVERLAP");
      overlap = e && e[0] == '1';
    }
    if (overlap) {
      if (cm->ctx != ctx) {
        ctx->err = "agp_comm belongs to another ctx (its collectives would run on another stream)";
        return AGP_ERR_INVALID;
      }
      AGPCHK(overlap_groups());
      arrive_epoch += 1;
      AGPCHK(comm_allreduce_groups(cm, stats, (int)sizeof(T), ov_off, ov_cnt, ov_ng, sizeof(T) == 8 ? AGP_F64 : AGP_F32, arrive_dev,
                                   arrive_epoch));
    } else
      AGPCHK(comm_sum(cm, stats, (int64_t)nl * stats_stride()));
    if (merge) {
      Latent& g = lat[0];
      pendp.on = true;
      s00_for.on = false;
      pendp.overlap = overlap;
      pendp.epoch = arrive_epoch;
      pendp.cm = cm;
      pendp.lr = (T)cur_lr();
      pendp.Kinv = kinv_step(g);
      pendp.kinv_mu0 = kinv_mu0_step(g);
      g.la_state = 1;  // La does not hold -2 eta2: whoever wants it rebuilds it from eta2 (after flush())
      g.xa_valid = false;
      g.post_valid = false;
      g.pred_valid = g.predvar_valid = false;
      n_opt += 1;
      return AGP_OK;
    }
    return step_global(false);
  }

  agp_status elbo_multi(agp_comm* cm, int mode, double* out) override {
    if (!out || !x_last || B_last <= 0) return AGP_ERR_INVALID;
    adopt_batch_shard(cm, mode);
    if (mo_sharded) {
      AGPCHK(mo_refresh_f());
      AGPCHK(comm_sum(cm, fall, (int64_t)2 * qtot * Bp));
    }
    double mine = 0.0;
    AGPCHK(elbo(x_last, ldx_last, y_last, idx_last, B_last, rho_last, 0, &mine));
    if (!cm || cm->world <= 1) {
      *out = mine;
      return AGP_OK;
    }
    // scalars travel as doubles through a small device buffer (scal_dev[56..59])
    double h[2] = {mode == AGP_SHARD_LATENT ? mine : e_data, mode == AGP_SHARD_LATENT ? 0.0 : kl_aug};
    HIPCHK(ctx, hipMemcpyAsync(scal_dev + 56, h, sizeof(double) * 2, hipMemcpyHostToDevice, st()));
    AGPCHK(comm_sum_typed(cm, scal_dev + 56, 2, AGP_F64));
    HIPCHK(ctx, hipMemcpyAsync(h, scal_dev + 56, sizeof(double) * 2, hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    *out = mode == AGP_SHARD_LATENT ? h[0] : rho_last * h[0] - kl_gauss_last - rho_last * h[1];
    return AGP_OK;
  }

  double* hy_tied = nullptr;  // [1 + D + m*D] doubles: summed gradient of the tied-Z mode
  agp_status hyper_step_multi(agp_comm* cm, int tied) override {
    if (!hy_k && !hy_z) return AGP_OK;
    if (cm && cm->world > 1 && bs_world > 1 && bs_world != cm->world) {
      ctx->err = "agp_svgp_hyper_step_multi: the handle's batch shard does not belong to this communicator";
      return AGP_ERR_INVALID;
    }
    if (mo_sharded) {  // the mixed data term of the gradient reads every latent's mean_f under the updated posterior
      AGPCHK(mo_refresh_f());
      AGPCHK(comm_sum(cm, fall, (int64_t)2 * qtot * Bp));
    }
    const int64_t ng = 1 + D + m * D;
    const bool batch_sharded = bs_world > 1;
    if (!tied && !batch_sharded) {
      hyper_multi_ok = true;
      const agp_status hs_ = hyper_step();
      hyper_multi_ok = false;
      return hs_;
    }
    if (!hy_tied) AGPCHK(dmalloc(ctx, &hy_tied, ng));
    if (!tied) {
      // batch-sharded handle, every latent its own kernel and Z: the data part of each latent's gradient is a sum over the ranks'
      // shards (all-reduced, 1 + D + m D doubles per latent), its Gaussian-KL part is replicated and enters with weight
      // 1 / world on every rank (k_hyper_gK) -- every rank then takes the identical ADAM step and the replicas stay together
      if (!cm || cm->world != bs_world) {
        ctx->err = "hyper step of a batch-sharded handle needs the communicator of the run";
        return AGP_ERR_INVALID;
      }
      for (int l = 0; l < nl; ++l) {
        AGPCHK(hypergrad(l, nullptr, nullptr, nullptr));
        HIPCHK(ctx, hipMemsetAsync(hy_tied, 0, sizeof(double) * ng, st()));
        HIPCHK(ctx, hipMemcpyAsync(hy_tied, hy_last.data(), sizeof(double) * (1 + D), hipMemcpyHostToDevice, st()));
        hipLaunchKernelGGL((k_acc_to_double<T>), grid1(m * D), dim3(256), 0, st(), m * D, (const T*)hy_dZ, hy_tied + 1 + D);
        LAUNCHCHK(ctx);
        AGPCHK(comm_sum_typed(cm, hy_tied, ng, AGP_F64));
        std::vector<double> hg(1 + D, 0.0);
        HIPCHK(ctx, hipMemcpyAsync(hg.data(), hy_tied, sizeof(double) * (1 + D), hipMemcpyDeviceToHost, st()));
        hipLaunchKernelGGL((k_double_to<T>), grid1(m * D), dim3(256), 0, st(), m * D, (const double*)(hy_tied + 1 + D), hy_dZ);
        LAUNCHCHK(ctx);
        HIPCHK(ctx, hipStreamSynchronize(st()));
        AGPCHK(hyper_apply_one(l, &hg, (const T*)hy_dZ));
      }
      return hyper_finish();
    }
    if (batch_sharded && (!cm || cm->world != bs_world)) {  // (the Gaussian-KL part enters with weight 1 / world: without the
      ctx->err = "tied hyper step of a batch-sharded handle needs the communicator of the run";  // all-reduce the step is wrong)
      return AGP_ERR_INVALID;
    }
    HIPCHK(ctx, hipMemsetAsync(hy_tied, 0, sizeof(double) * ng, st()));
    std::vector<double> hs(1 + D, 0.0);
    for (int l = 0; l < nl; ++l) {
      AGPCHK(hypergrad(l, nullptr, nullptr, nullptr));
      for (int64_t i = 0; i < 1 + D; ++i) hs[i] += hy_last[i];
      hipLaunchKernelGGL((k_acc_to_double<T>), grid1(m * D), dim3(256), 0, st(), m * D, (const T*)hy_dZ, hy_tied + 1 + D);
      LAUNCHCHK(ctx);
    }
    HIPCHK(ctx, hipMemcpyAsync(hy_tied, hs.data(), sizeof(double) * (1 + D), hipMemcpyHostToDevice, st()));
    AGPCHK(comm_sum_typed(cm, hy_tied, ng, AGP_F64));
    HIPCHK(ctx, hipMemcpyAsync(hs.data(), hy_tied, sizeof(double) * (1 + D), hipMemcpyDeviceToHost, st()));
    hipLaunchKernelGGL((k_double_to<T>), grid1(m * D), dim3(256), 0, st(), m * D, (const double*)(hy_tied + 1 + D), hy_dZ);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st()));
    for (int l = 0; l < nl; ++l) AGPCHK(hyper_apply_one(l, &hs, (const T*)hy_dZ));
    return hyper_finish();
  }

  agp_status predict_multi(agp_comm* cm, int what, const void* xt, int64_t ldx, int64_t nt, void* mu, void* var,
                           const double* nodes, const double* weights, int nn) override {
    if (what < 0 || what > 2 || !mu || (what == 2 && !var)) return AGP_ERR_INVALID;
    if (!mo_sharded) {  // nothing is sharded on the prediction side: the plain calls apply
      if (what == 0) return predict_f(xt, ldx, nt, mu, var);
      if (what == 1) return predict_y(xt, ldx, nt, mu);
      return proba_y(xt, ldx, nt, nodes, weights, nn, mu, var);
    }
    void* v = what == 1 ? nullptr : var;
    AGPCHK(predict_f(xt, ldx, nt, mu, v));  // partial mix over the owned columns of A
    AGPCHK(comm_sum(cm, mu, (int64_t)nT * nt));
    if (v) AGPCHK(comm_sum(cm, v, (int64_t)nT * nt));
    if (what == 0) return AGP_OK;
    return mo_predict_from_f(nt, what == 1 ? 0 : 1, mu, var, nodes, weights, nn);
  }

  agp_status proba_y_single(const void* xt, int64_t ldx, int64_t nt, const double* nodes, const double* weights, int nn,
                            void* o0, void* o1) {
    AGPCHK(predict_f(xt, ldx, nt, pmu, pvar));
    if (lp.kind == AGP_LIK_GAUSSIAN) {
      if (!o1) return AGP_ERR_INVALID;
      T s2 = lp.p0;
      if (lp.noise_dev) {  // the optimised noise lives on the device (compute_proba adds noise(l), gaussian.jl:41-45)
        double v = 0.0;
        AGPCHK(get_lik_param(&v));
        s2 = (T)v;
      }
      hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu, (const T*)pvar, s2, 0, (T*)o0,
                         (T*)o1);
    } else if (lp.kind == AGP_LIK_STUDENTT) {
      if (!o1) return AGP_ERR_INVALID;
      const double nu = desc.lik.p0, sg = desc.lik.p1;
      hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu, (const T*)pvar,
                         (T)(nu * sg * sg / (2.0 * (nu / 2.0 - 1.0))), 1, (T*)o0, (T*)o1);
    } else if (lp.kind == AGP_LIK_LOGISTIC) {
      if (!o1 || !nodes || !weights || nn <= 0) return AGP_ERR_INVALID;
      AGPCHK(upload_gh(nodes, weights, nn));
      hipLaunchKernelGGL((k_proba_logistic<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu, (const T*)pvar, nn,
                         (const double*)gh_dev, (const double*)(gh_dev + nn), (T*)o0, (T*)o1);
    } else if (lp.kind == AGP_LIK_LAPLACE) {  // laplace.jl:48-52
      if (!o1) return AGP_ERR_INVALID;
      hipLaunchKernelGGL((k_proba_regression<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu, (const T*)pvar,
                         (T)(2.0 * desc.lik.p0 * desc.lik.p0), 1, (T*)o0, (T*)o1);
    } else if (lp.kind == AGP_LIK_HETEROSCEDASTIC) {
      if (!o1) return AGP_ERR_INVALID;
      hipLaunchKernelGGL((k_proba_hetero<T>), grid1(nt), dim3(256), 0, st(), nt, nt, (const T*)pmu, (const T*)pvar,
                         (const T*)lam_dev, (T*)o0, (T*)o1);
    } else if (lp.kind == AGP_LIK_BAYESIANSVM || lp.kind == AGP_LIK_POISSON || lp.kind == AGP_LIK_NEGBINOMIAL) {
      if (!o1 || !nodes || !weights || nn <= 0) return AGP_ERR_INVALID;
      AGPCHK(upload_gh(nodes, weights, nn));
      const int link = lp.kind == AGP_LIK_BAYESIANSVM ? 1 : (lp.kind == AGP_LIK_POISSON ? 2 : 3);
      hipLaunchKernelGGL((k_proba_gh<T>), grid1(nt), dim3(256), 0, st(), nt, (const T*)pmu, (const T*)pvar, nn,
                         (const double*)gh_dev, (const double*)(gh_dev + nn), link, desc.lik.p0,
                         lp.kind == AGP_LIK_POISSON ? (const T*)lam_dev : (const T*)nullptr, (T*)o0, (T*)o1);
    } else if (lp.kind == AGP_LIK_SOFTMAX) {
      hipLaunchKernelGGL((k_proba_softmax<T>), grid1(nt), dim3(256), 0, st(), nt, nl, nt, (const T*)pmu, (T*)o0);
    } else {
      hipLaunchKernelGGL((k_proba_lsm<T>), grid1(nt), dim3(256), 0, st(), nt, nl, nt, (const T*)pmu, (T*)o0);
    }
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
};

// ---- full model (AGP_FLAG_FULL: VGP, kappa = I, m = N, Z = the training inputs) -------------------------------------------
// VGP(X, y, kernel, likelihood, AnalyticVI())  src/models/VGP.jl:36-85, Float64 only: the SVGP handle without K_nm, kappa, K~
struct Vgp : Svgp<double> {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("full models (AGP_FLAG_FULL, VGP) are not supported: the streamed ELBO is the sparse model's");
  }
  using T = double;
  T* vgp_part = nullptr;  // [part_sets()][2][ns][mp] partial column sums of k_vgp_colstats (colstats_part)
  virtual int part_sets() const { return 1; }  // one set serves every latent in turn (Vgp, Gp); one per latent in Movgp
  Vgp() { sparse_bufs = false; }
  ~Vgp() override {
    if (vgp_part) dfree(vgp_part);
  }
  // what a full model takes: AnalyticVI, max_batch = m = N and all of its latents on this handle
  agp_status check_full() {
    if (desc.stochastic || Bmax != m || desc.latent_offset != 0) {
      ctx->err = "AGP_FLAG_FULL: the full model takes AnalyticVI, max_batch = m = N and all of its latents on one handle";
      return AGP_ERR_INVALID;
    }
    return AGP_OK;
  }
  agp_status check_desc() override {
    AGPCHK(Svgp<T>::check_desc());
    AGPCHK(check_full());
    if (lp.kind == AGP_LIK_GAUSSIAN) {  // VGP.jl:54-56
      ctx->err = "For a Gaussian Likelihood you should directly use the `GP` model or the `SVGP` model for large datasets";
      return AGP_ERR_UNSUPPORTED;
    }
    return AGP_OK;
  }
  // the ns row slices of a k_vgp_colstats pass (fixed by mp) and their partial sums in vgp_part (allocated by the first pass)
  agp_status colstats_part(int* ns) {
    const int64_t ntc = mp / TILE;
    *ns = (int)std::max<int64_t>(1, std::min<int64_t>(ntc, (2048 + ntc - 1) / ntc));
    if (!vgp_part) AGPCHK(dmalloc(ctx, &vgp_part, 2 * (int64_t)*ns * mp * part_sets()));
    return AGP_OK;
  }
  void record_batch(const void* y, double rho) {  // every step's batch: the whole training set (x = Z, idx = NULL, B = N)
    x_last = lat[0].Z;
    y_last = y;
    idx_last = nullptr;
    B_last = m;
    ldx_last = D;
    rho_last = rho;
  }
  // factor -2 eta2 with its inverse Xa and v = Xa eta1 (the [eta1' ; 0] extension block of the factorisation) -- no Sigma, no kappa
  // rows: the blocked / task-graph factorisation with its X = L^-1 output; a lost task-graph dependency is redone by its plain
  // in-stream fallback (k_chol_safe), which rebuilds A = -2 eta2 and the eta1 row from the same sources
  agp_status vgp_factor(Latent& g) {
    if (g.la_state != 0) {  // La holds a factor: rebuild -2 eta2
      hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)g.eta2, mp, mp, mp, g.La, mp, mp, mp, T(1), T(-2));
      LAUNCHCHK(ctx);
    }
    SafeSrc<T> src{};
    src.Bq = 0;
    src.eta1[0] = g.eta1;
    src.eta2[0] = g.eta2;
    src.want_x = 1;
    AGPCHK(timing_begin());
    PotrfReq<T> rq{};
    rq.A = g.La, rq.ld = mp, rq.n = mp, rq.X = g.Xa, rq.ldx = mp, rq.Dg = g.DgA, rq.E = g.Wbuf, rq.lde = mp, rq.ne = 1, rq.do_x = 1;
    rq.info_dev = info_dev, rq.nvalid = m, rq.erow = g.eta1, rq.want_l = false, rq.safe = &src;
    AGPCHK(potrf_fused<T>(ctx, rq));
    AGPCHK(timing_end(chol_use_dag(ctx, mp / TILE, 1) ? 1 : chol_launch_count(mp / TILE, 1)));
    g.la_state = 1;
    g.xa_valid = true;
    g.xa_epoch += 1;
    g.sigma_epoch = -1;
    HIPCHK(ctx, hipMemcpyAsync(g.v, g.Wbuf, sizeof(T) * mp, hipMemcpyDeviceToDevice, st()));
    g.v_epoch = g.xa_epoch;
    return AGP_OK;
  }
  // what every local phase of a full model starts with: the whole training set (idx = NULL, B = N), the kernel matrices when the
  // kernel moved, the previous step's deferred fallback
  agp_status step_begin(const void* y, const int64_t* idx, int64_t B, bool fresh) {
    if (idx != nullptr || B != m) {
      ctx->err = "full model (AGP_FLAG_FULL): steps and ELBO evaluations run on the whole training set (idx = NULL, B = N = m)";
      return AGP_ERR_BAD_BATCH;
    }
    if (!y) return AGP_ERR_INVALID;
    lsm_finished = false;
    for (auto& g : lat) g.C_valid = false;
    refresh_lazy = !fresh;
    const agp_status rks = refresh_K();
    refresh_lazy = false;
    AGPCHK(rks);
    return run_deferred_safe();
  }
  // one latent's factor of -2 eta2 with its inverse when it is not at hand, v = Xa eta1, and the k_vgp_colstats pass into the ns
  // slices part[0][ns][mp] (sum Xa^2) and part[1][ns][mp] (sum Xa v)
  agp_status colstats(Latent& g, int ns, T* part) {
    const int64_t ntc = mp / TILE, rows = (mp + ns - 1) / ns;
    if (!(g.la_state == 1 && g.xa_valid)) AGPCHK(vgp_factor(g));
    if (g.v_epoch != g.xa_epoch) {
      hipLaunchKernelGGL((k_trmv_lower<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Xa, mp, mp, (const T*)g.eta1, g.v);
      g.v_epoch = g.xa_epoch;
    }
    hipLaunchKernelGGL((k_vgp_colstats<T>), dim3((unsigned)ntc, (unsigned)ns), dim3(256), 0, st(), mp, (const T*)g.Xa,
                       (const T*)g.v, rows, part, part + (int64_t)ns * mp);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  // update_parameters!(::VGP) first half (training.jl:140-144): local_updates! on mean_f = mu, var_f = diag Sigma of the current
  // posterior (latentgp.jl:171-189).  The factor of -2 eta2 and its inverse come from the factorisation (or from the last
  // materialize(), which left them); mu and diag Sigma from one pass over the lower triangle of Xa (k_vgp_colstats), which feeds the
  // point-wise likelihood update directly.  The whole training set every time: idx = NULL, B = N.
  agp_status step_local(const void*, int64_t, const void* y, const int64_t* idx, int64_t B, double rho, bool fresh) override {
    AGPCHK(step_begin(y, idx, B, fresh));
    int ns = 0;
    AGPCHK(colstats_part(&ns));
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      AGPCHK(colstats(g, ns, vgp_part));
      hipLaunchKernelGGL((k_vgp_local<T>), grid1(m), dim3(256), 0, st(), m, mp, ns, (const T*)vgp_part,
                         (const T*)(vgp_part + (int64_t)ns * mp), (T)rho, lp, (const T*)y, Kt + l * Bp, muf + l * Bp,
                         varf + l * Bp, cbuf + l * Bp, theta + l * Bp, rbuf + l * Bp, wbuf + l * Bp, (const T*)lam_dev,
                         gamma + l * Bp);
      LAUNCHCHK(ctx);
    }
    AGPCHK(lik_tail(y, idx, B, rho, fresh));
    record_batch(y, rho);
    return AGP_OK;
  }
  // natural_gradient! + global_update! of the full model (analyticVI.jl:126-140, inference.jl:25-28): eta and La = -2 eta2 by one
  // streaming pass (k_vgp_eta); the factorisation itself is left to whoever needs the new posterior next (the next step's local
  // phase, materialize())
  agp_status step_finish() override {
    AGPCHK(lsm_finish());
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      hipLaunchKernelGGL((k_vgp_eta<T>), dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, st(), m, mp,
                         (const T*)kinv_step(g), (const T*)(rbuf + l * Bp), (const T*)(wbuf + l * Bp), (const T*)kinv_mu0_step(g),
                         g.eta2, g.La, g.eta1);
      LAUNCHCHK(ctx);
      g.la_state = 0;
      g.xa_valid = false;
      g.C_valid = false;
      g.post_valid = false;
      g.pred_valid = g.predvar_valid = false;
    }
    n_opt += 1;
    return AGP_OK;
  }
  // mean_f / var_f under the UPDATED posterior for objective(model, state, y): mu and diag Sigma of the materialised posterior
  agp_status posterior_f(int64_t) override {
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      AGPCHK(materialize(g));
      hipLaunchKernelGGL((k_vgp_diag<T>), grid1(m), dim3(256), 0, st(), m, mp, (const T*)g.Sigma, (const T*)g.mu, emuf + l * Bp,
                         evarf + l * Bp);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }
  // update_hyperparameters!(::VGP) (autotuning.jl:49-85): only the Gaussian KL depends on the kernel, through Apred and K^-1 (mu - mu0).
  // X is never optimised: no dZ.
  agp_status hypergrad(int l, double* dvar, double* dscale, void* dZ_out) override {
    AGPCHK(check_hypergrad(l, dZ_out));
    Latent& g = lat[l];
    AGPCHK(hyper_alloc());
    AGPCHK(refresh_K());
    AGPCHK(ensure_pred(g, true));  // Sigma, mu, K^-1 mu, Apred = K^-1 - K^-1 Sigma K^-1
    return kernel_grad(g, g.Apred, g.apred, g.kinv_mu0, dvar, dscale);
  }
  // what the hyper-gradient of a full model refuses: an unknown latent, no step yet, dZ, the ExponentialKernel
  agp_status check_hypergrad(int l, const void* dZ_out) {
    if (l < 0 || l >= nl || B_last <= 0) return AGP_ERR_INVALID;
    if (dZ_out) {
      ctx->err = "full model (AGP_FLAG_FULL): the training inputs are not optimised (no dZ)";
      return AGP_ERR_UNSUPPORTED;
    }
    if (lat[l].k.kind == AGP_K_EXPONENTIAL) {
      ctx->err = "hyper-gradient: ExponentialKernel is not differentiable at zero distance";
      return AGP_ERR_UNSUPPORTED;
    }
    return AGP_OK;
  }
  // G_K = ((a - a0)(a - a0)' - Apred) / 2, a0 = kinv_mu0 or 0 (k_vgp_gK), then the backward pass through kernelmatrix(k, X) with
  // both operands X (G_K symmetric: twice the second-argument part) and its reduction into hy_g
  agp_status kernel_grad(Latent& g, const T* Apred, const T* a, const T* kinv_mu0, double* dvar, double* dscale) {
    n_hgrad += 1;
    hipLaunchKernelGGL((k_vgp_gK<T>), grid2(mp, mp), blk2, 0, st(), m, mp, Apred, a, kinv_mu0, Tw2);
    tw2_kis_of = -1;
    dim3 gk((unsigned)(mp / TILE), (unsigned)(mp / HB_RT));
    const int64_t tiles = (int64_t)gk.x * gk.y;
    hipLaunchKernelGGL((k_kernel_backward<T>), gk, dim3(NTHREADS), 0, st(), (const T*)g.Z, D, (const int64_t*)nullptr, m,
                       (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g), (const T*)Tw2, mp, hy_pvar, hy_pscale,
                       hy_pZ, mp);
    hipLaunchKernelGGL((k_hyper_reduce<T>), dim3((unsigned)(D + 1 + (m * D + 255) / 256)), dim3(256), 0, st(), tiles, D,
                       (const double*)hy_pvar, (const double*)hy_pscale, hy_g, 1.0, 1, (int64_t)gk.y, m, mp, (const T*)hy_pZ,
                       hy_dZ, T(2), (const T*)nullptr, (int64_t)0, 0.0);
    LAUNCHCHK(ctx);
    return hypergrad_to_host(dvar, dscale);
  }
};

// ---- multi-output full model (AGP_FLAG_FULL with AGP_LIK_MULTIOUTPUT: MOVGP, src/models/MOVGP.jl) ------------------------------
// MOVGP(X, y, kernel, likelihoods, AnalyticVI(), num_latent): Q full latents on the training inputs, mixed by A into one output per
// task (update_parameters!(::MOVGP), training.jl:146-151).  The posterior side of a step is Vgp's, latent by latent; the likelihood
// side is the multi-output machinery of the sparse model (mo_local: update_A!, the mixed local updates, r / w per latent), fed with
// mean_f[q] = mu_q, var_f[q] = diag Sigma_q.  ELBO, predictions, hyper step (only the Gaussian KL depends on a latent's kernel),
// state export: the inherited ones, which reach this class through step_local / posterior_f / hypergrad.
struct Movgp : Vgp {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("multi-output full models (AGP_FLAG_FULL with AGP_LIK_MULTIOUTPUT, MOVGP) are not supported");
  }
  agp_status check_desc() override {
    AGPCHK(Svgp<T>::check_desc());
    return check_full();
  }
  // update_A! on (mu_q, diag Sigma_q) of the current posterior and the local variables of the step before, the local update of every
  // task on the mixed (sum_q A_tq mu_q, sum_q A_tq^2 diag Sigma_q), then the mixed gradients per latent (analyticVI.jl:48-111)
  agp_status step_local(const void*, int64_t, const void* y, const int64_t* idx, int64_t B, double rho, bool fresh) override {
    if (!mo) {
      ctx->err = "multi-output handle: call agp_svgp_set_multioutput first";
      return AGP_ERR_INVALID;
    }
    AGPCHK(step_begin(y, idx, B, fresh));
    int ns = 0;
    AGPCHK(colstats_part(&ns));
    const int64_t set = 2 * (int64_t)ns * mp;
    for (int l = 0; l < nl; ++l) AGPCHK(colstats(lat[l], ns, vgp_part + l * set));
    hipLaunchKernelGGL((k_movgp_fstats<T>), dim3((unsigned)((m + 255) / 256), (unsigned)nl), dim3(256), 0, st(), m, mp, ns,
                       (const T*)vgp_part, Bp, muf, varf);
    LAUNCHCHK(ctx);
    AGPCHK(mo_local(y, nullptr, m, rho, !fresh, muf, varf));
    record_batch(y, rho);
    return AGP_OK;
  }
  int part_sets() const override { return nl; }  // k_movgp_fstats reads every latent's slices
  agp_status pathwise_draw(int, int, uint64_t, int64_t, agp_pathwise**) override {
    return pathwise_refused("multi-output handles (MOSVGP, MOVGP) are not supported: draw from single-output models");
  }
};

// ---- exact GP (AGP_FLAG_FULL | AGP_FLAG_EXACT: GP(X, y, kernel) with Analytic(), src/models/GP.jl, analytic.jl) ------------
// K + jitt I is kept unfactored in g.L (refreshed only when the kernel moved: numerically the reference's recompute every
// iteration).  A step factors Sigma = K + sigma2 I in g.La with its inverse g.Xa = L^-1 and the extension row r = y - mu0 (g.eta1),
// whose image v = L^-1 r lands in g.v; alpha = Sigma^-1 r goes to g.mu, diag Sigma^-1 to gp_dinv, log p to gp_out[4], and the
// sigma2 the factor used to gp_s2.  Sigma^-1 (g.Apred) and Sigma (g.Sigma) are formed on demand, once per factor.
struct Gp : Vgp {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("exact GP regression (AGP_FLAG_EXACT, GP) is not supported");
  }
  bool gp_have_r = false;       // g.eta1 holds r (from the first step)
  bool gp_valid = false;        // the factor, alpha and log p belong to the current K
  bool gp_s2_fresh = false;     // ... and to the current sigma2 (no noise step since)
  bool gp_sinv_valid = false, gp_sigma_valid = false;
  T* gp_dinv = nullptr;         // diag Sigma^-1
  T* gp_m0v = nullptr;          // L^-1 mu0 (the reference's y' Sigma^-1 y with a prior mean)
  T* gp_s2 = nullptr;           // sigma2 of the current factor
  double* gp_part = nullptr;    // [6][nb] partial sums of k_gp_partial
  double* gp_out = nullptr;     // [alpha' alpha, tr Sigma^-1, r' alpha, sum log L_ii, log p]
  bool gp_ref() const { return desc.elbo_mode == AGP_ELBO_REFERENCE; }
  ~Gp() override {
    for (T* p : {gp_dinv, gp_m0v, gp_s2})
      if (p) dfree(p);
    for (double* p : {gp_part, gp_out})
      if (p) dfree(p);
  }
  // the generic checks, then GP(X, y, kernel)'s, then the shape of a full model
  agp_status check_desc() override {
    AGPCHK(Svgp<T>::check_desc());
    if (lp.kind != AGP_LIK_GAUSSIAN || nl != 1) {  // GP(X, y, kernel): GP.jl:37-65
      ctx->err = "AGP_FLAG_EXACT: exact GP regression takes AGP_FLAG_FULL, one latent and a Gaussian likelihood";
      return AGP_ERR_UNSUPPORTED;
    }
    return check_full();
  }
  agp_status init() override {
    AGPCHK(Vgp::init());
    AGPCHK(dmalloc(ctx, &gp_dinv, mp));
    AGPCHK(dmalloc(ctx, &gp_m0v, mp));
    AGPCHK(dmalloc(ctx, &gp_s2, 1));
    AGPCHK(dmalloc(ctx, &gp_part, 6 * ((mp + 255) / 256)));
    AGPCHK(dmalloc(ctx, &gp_out, 8));
    return AGP_OK;
  }
  // compute_Ks (training.jl:167-171, latentgp.jl:201-203): K = kernelmatrix(k, X) + jitt I, identity in the padding
  agp_status refresh_K() override {
    Latent& g = lat[0];
    if (!g.K_stale) return AGP_OK;
    AGPCHK(ensure_zsc(g));
    (void)launch_kernelmatrix<T>(ctx, st(), (const T*)g.Z, D, (const int64_t*)nullptr, m, (const T*)g.Z, D, m, D,
                                 (const T*)g.scales, g.k.kind, kvar(g), g.L, mp, mp, mp, 1, (T)jitter, (const T*)nullptr, (T*)nullptr,
                                 (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
    LAUNCHCHK(ctx);
    g.K_stale = false;
    gp_valid = false;
    gp_sinv_valid = gp_sigma_valid = false;
    g.pred_valid = g.predvar_valid = false;
    return AGP_OK;
  }
  // compute_Ks + post_step! (training.jl:107-108, GP.jl:80-85): K, then Sigma and alpha with the current sigma2
  agp_status refresh_K_explicit() override {
    AGPCHK(refresh_K());
    return (gp_have_r && !(gp_valid && gp_s2_fresh)) ? gp_factor(nullptr, false) : AGP_OK;
  }

  // analytic_updates (analytic.jl:36-51) / post_step! (GP.jl:80-85): Sigma = K + sigma2 I, alpha = Sigma \ (y - mu0), log p; with
  // noise_step (and opt_noise) the ADAM step on log sigma2 that follows.  y = NULL: r from the last step.  No host synchronisation.
  agp_status gp_factor(const T* y, bool noise_step) {
    if (!y && !gp_have_r) {
      ctx->err = "exact GP (AGP_FLAG_EXACT): no step has been taken yet (the targets arrive with agp_svgp_cavi_step)";
      return AGP_ERR_INVALID;
    }
    AGPCHK(refresh_K());
    Latent& g = lat[0];
    int ns = 0;
    AGPCHK(colstats_part(&ns));
    const int64_t ntc = mp / TILE;
    hipLaunchKernelGGL((k_gp_shift<T>), dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, st(), m, mp, (const T*)g.L,
                       (const T*)lam_dev, y, (const T*)g.mu0, g.La, y ? g.eta1 : (T*)nullptr, gp_s2);
    LAUNCHCHK(ctx);
    if (y) gp_have_r = true;
    // a lost task-graph dependency: the in-stream fallback rebuilds Sigma from K and the sigma2 word, the row from r
    SafeSrc<T> src{};
    src.Bq = 0;
    src.eta1[0] = g.eta1;
    src.want_x = 1;
    src.gpK = g.L;
    src.gps2 = lam_dev;
    src.mz = m;
    AGPCHK(timing_begin());
    PotrfReq<T> rq{};
    rq.A = g.La, rq.ld = mp, rq.n = mp, rq.X = g.Xa, rq.ldx = mp, rq.Dg = g.DgA, rq.E = g.Wbuf, rq.lde = mp, rq.ne = 1, rq.do_x = 1;
    rq.info_dev = info_dev, rq.nvalid = m, rq.erow = g.eta1, rq.want_l = false, rq.safe = &src;
    AGPCHK(potrf_fused<T>(ctx, rq));
    AGPCHK(timing_end(chol_use_dag(ctx, mp / TILE, 1) ? 1 : chol_launch_count(mp / TILE, 1)));
    HIPCHK(ctx, hipMemcpyAsync(g.v, g.Wbuf, sizeof(T) * mp, hipMemcpyDeviceToDevice, st()));
    const bool ref_m0 = gp_ref() && g.mu0;
    if (ref_m0)
      hipLaunchKernelGGL((k_trmv_lower<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Xa, mp, mp, (const T*)g.mu0, gp_m0v);
    const int64_t rows = (mp + ns - 1) / ns;
    hipLaunchKernelGGL((k_vgp_colstats<T>), dim3((unsigned)ntc, (unsigned)ns), dim3(256), 0, st(), mp, (const T*)g.Xa, (const T*)g.v,
                       rows, vgp_part, vgp_part + (int64_t)ns * mp);
    const int nb = (int)((mp + 255) / 256);
    hipLaunchKernelGGL((k_gp_partial<T>), dim3(nb), dim3(256), 0, st(), m, mp, ns, (const T*)vgp_part,
                       (const T*)(vgp_part + (int64_t)ns * mp), (const T*)g.eta1, (const T*)g.DgA, (const T*)g.mu0,
                       ref_m0 ? (const T*)gp_m0v : (const T*)nullptr, g.mu, gp_dinv, gp_part);
    const bool step_noise = noise_step && lp.noise_dev;
    hipLaunchKernelGGL((k_gp_finish<T>), dim3(1), dim3(256), 0, st(), nb, (const double*)gp_part, m, gp_ref() ? 1 : 0, noise_eta,
                       step_noise ? noise_adam : (double*)nullptr, lam_dev, gp_out);
    LAUNCHCHK(ctx);
    gp_valid = true;
    gp_s2_fresh = !step_noise;
    gp_sinv_valid = gp_sigma_valid = false;
    g.pred_valid = g.predvar_valid = false;
    return AGP_OK;
  }
  agp_status step_local(const void*, int64_t, const void* y, const int64_t* idx, int64_t B, double, bool) override {
    if (idx != nullptr || B != m) {
      ctx->err = "exact GP (AGP_FLAG_EXACT): steps run on the whole training set (idx = NULL, B = N = m)";
      return AGP_ERR_BAD_BATCH;
    }
    if (!y) return AGP_ERR_INVALID;
    AGPCHK(gp_factor((const T*)y, true));
    record_batch(y, 1.0);
    return AGP_OK;
  }
  agp_status step_finish() override {  // (the whole Analytic step ran in step_local)
    n_opt += 1;
    return AGP_OK;
  }
  // Sigma^-1 = L^-T L^-1 of the current factor (the predictor's Apred, the hyper-gradient's)
  agp_status gp_sinv() {
    Latent& g = lat[0];
    if (!gp_valid) AGPCHK(gp_factor(nullptr, false));
    if (gp_sinv_valid) return AGP_OK;
    if (!g.Apred) AGPCHK(dmalloc(ctx, &g.Apred, mp * mp));
    AGPCHK(xtx_padded<T>(ctx, g.Xa, mp, mp, g.Apred, mp));
    gp_sinv_valid = true;
    return AGP_OK;
  }
  // predictions.jl:6-23: mu* = K*n alpha (mu0 not added back), var* = k** + jitt - diag(K*n Sigma^-1 Kn*): the streaming predictor
  // with apred = alpha, Apred = Sigma^-1
  agp_status ensure_pred(Latent& g, bool need_var) override {
    if (!gp_valid) AGPCHK(gp_factor(nullptr, false));
    if (!g.apred) AGPCHK(dmalloc(ctx, &g.apred, mp));
    if (!g.pred_valid) {
      HIPCHK(ctx, hipMemcpyAsync(g.apred, g.mu, sizeof(T) * mp, hipMemcpyDeviceToDevice, st()));
      g.pred_valid = true;
    }
    if (need_var && !g.predvar_valid) {
      AGPCHK(gp_sinv());
      g.predvar_valid = true;
    }
    return AGP_OK;
  }
  // objective(m::GP, _, y) = log_py (GP.jl:87-92) of the stored posterior.  y binds the targets of a handle that has taken no step
  // yet (a reloaded model: post_step! with the restored sigma2); afterwards it is not read.
  agp_status elbo(const void*, int64_t, const void* y, const int64_t*, int64_t, double, int, double* out) override {
    if (!out) return AGP_ERR_INVALID;
    if (y && !gp_have_r) AGPCHK(gp_factor((const T*)y, false));
    else if (!gp_valid) AGPCHK(gp_factor(nullptr, false));
    HIPCHK(ctx, hipMemcpyAsync(out, gp_out + 4, sizeof(double), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    return AGP_OK;
  }
  // mu <- alpha, sigma <- Sigma (the posterior of GP.jl: Posterior(Sigma, alpha)); there are no natural parameters
  agp_status get_state(int l, void* mu, void* sigma, void* eta1, void* eta2) override {
    if (l < 0 || l >= nl) return AGP_ERR_INVALID;
    if (eta1 || eta2) {
      ctx->err = "exact GP (AGP_FLAG_EXACT): the posterior has no natural parameters (eta1 / eta2 must be NULL)";
      return AGP_ERR_UNSUPPORTED;
    }
    Latent& g = lat[0];
    if ((mu || sigma) && !gp_valid) AGPCHK(gp_factor(nullptr, false));
    if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, g.mu, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    if (sigma) {
      if (!gp_sigma_valid) {
        hipLaunchKernelGGL((k_gp_shift<T>), dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, st(), m, mp, (const T*)g.L,
                           (const T*)gp_s2, (const T*)nullptr, (const T*)nullptr, g.Sigma, (T*)nullptr, (T*)nullptr);
        LAUNCHCHK(ctx);
        gp_sigma_valid = true;
      }
      HIPCHK(ctx, hipMemcpy2DAsync(sigma, sizeof(T) * m, g.Sigma, sizeof(T) * mp, sizeof(T) * m, m, hipMemcpyDeviceToDevice, st()));
    }
    return AGP_OK;
  }
  agp_status set_state(int, const void*, const void*) override {
    ctx->err = "exact GP (AGP_FLAG_EXACT): the posterior follows from K, sigma2 and y; it has no natural parameters to set";
    return AGP_ERR_UNSUPPORTED;
  }
  // G1 corrected: d log p / d theta = tr((alpha alpha' - Sigma^-1) dK/dtheta) / 2 at the Sigma of the last step (kernel_grad with
  // Apred = Sigma^-1, a = alpha).  Reference mode: the reference's gradient is `nothing` (zeros here).
  agp_status hypergrad(int l, double* dvar, double* dscale, void* dZ_out) override {
    AGPCHK(check_hypergrad(l, dZ_out));
    if (gp_ref()) {
      if (dvar) *dvar = 0.0;
      if (dscale)
        for (int64_t d = 0; d < D; ++d) dscale[d] = 0.0;
      return AGP_OK;
    }
    AGPCHK(hyper_alloc());
    AGPCHK(gp_sinv());
    Latent& g = lat[0];
    return kernel_grad(g, g.Apred, g.mu, nullptr, dvar, dscale);
  }
  // G1 in the reference mode: the kernel gradient is `nothing` -- kernel and optimiser state untouched, a caller-supplied gradient
  // moves nothing either (after the argument checks of every handle)
  agp_status hyper_step() override { return gp_ref() ? AGP_OK : Vgp::hyper_step(); }
  agp_status hyper_apply(int l, const double* dvar, const double* dscale, const void* dZ) override {
    if (!gp_ref()) return Vgp::hyper_apply(l, dvar, dscale, dZ);
    return (l < 0 || l >= nl || !dvar || !dscale) ? AGP_ERR_INVALID : AGP_OK;
  }
  agp_status set_lik_param(double v) override {
    AGPCHK(Vgp::set_lik_param(v));
    gp_s2_fresh = false;  // (the closing refresh_K_explicit refactors with the new sigma2)
    return AGP_OK;
  }
  // pathwise sampling: V = alpha 1' - Sigma_y^-1 (Phi(X) W + sigma E) with alpha, Sigma_y^-1 and sigma2 of the current factor
  agp_status pathwise_latent(agp_pathwise& p, int l) override {
    Latent& g = lat[0];
    if (!gp_valid) AGPCHK(gp_factor(nullptr, false));
    AGPCHK(gp_sinv());
    double s2 = 0.0;
    HIPCHK(ctx, hipMemcpyAsync(&s2, gp_s2, sizeof(double), hipMemcpyDeviceToHost, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));
    PwScratch sc;
    double* PW = nullptr;
    AGPCHK(sc.get(ctx, &PW, mp * p.Sp));
    AGPCHK(pw_phi_W(p, l, PW));
    hipLaunchKernelGGL(k_pw_add_noise, grid2(m, p.S), blk2, 0, st(), m, (int64_t)p.S, p.Sp, std::sqrt(s2), (const double*)p.lat[l].E, PW);
    LAUNCHCHK(ctx);
    AGPCHK(pw_gemm_tn(ctx, PW, p.Sp, g.Apred, mp, p.Sp, mp, mp, p.lat[l].WV + p.Lp, p.ldw));
    hipLaunchKernelGGL(k_pw_gp_finish, grid2(p.S, m), blk2, 0, st(), m, (int64_t)p.S, p.ldw, (const double*)g.mu, p.lat[l].WV + p.Lp);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st()));  // the scratch goes out of scope
    return AGP_OK;
  }
};

// ---- Gibbs-sampled full model (AGP_FLAG_FULL | AGP_FLAG_SAMPLED: MCGP(X, y, kernel, likelihood, GibbsSampling())) --------------
// src/models/MCGP.jl, src/inference/gibbssampling.jl, src/training/sampling.jl.  The state of the chain is f (kept in g.mu) and the
// sweep counter t.  One sweep: k_gibbs_local draws the local variables at f and writes theta and the expectation gradients where
// k_vgp_local writes them; k_vgp_eta forms eta1 and -2 eta2 = inv(K) + 2 Diagonal(grad_E_Sigma); Vgp::vgp_factor leaves Xa = L^-1 and
// v = Xa eta1; k_gibbs_f / k_gibbs_fsum draw f = Xa' (v + z) ~ N(Sigma eta1, Sigma).  Nothing between sweeps waits for the host.
struct Mcgp : Vgp {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("Gibbs-sampled models (AGP_FLAG_SAMPLED, MCGP) are not supported");
  }
  int64_t gibbs_t = 0;    // sweeps taken so far: the counter word of the next sweep's draws
  bool swept = false;     // Xa belongs to a sweep (else Sigma = I, latentgp.jl:81-86)
  T *mc_Fs = nullptr, *mc_G = nullptr, *mc_Fstar = nullptr;  // prediction: padded samples, F K^-1, F* of one block of test points
  int64_t mc_sp = 0;
  static constexpr int64_t MC_MAX_SAMPLES = 65536;  // (the workspace holds F K^-1 for all samples of a call: 2 x 8 N bytes each)
  ~Mcgp() override {
    for (T* p : {mc_Fs, mc_G, mc_Fstar})
      if (p) dfree(p);
  }
  static const char* supported() { return "Gibbs sampling on the device runs for the Logistic, StudentT and NegBinomial likelihoods"; }
  agp_status check_desc() override {
    AGPCHK(Svgp<T>::check_desc());
    AGPCHK(check_full());
    if (lp.kind == AGP_LIK_GAUSSIAN) {  // MCGP.jl:54-56
      ctx->err = "For a Gaussian Likelihood you should directly use the `GP` model or the `SVGP` model for large datasets";
      return AGP_ERR_UNSUPPORTED;
    }
    if (lp.kind != AGP_LIK_LOGISTIC && lp.kind != AGP_LIK_STUDENTT && lp.kind != AGP_LIK_NEGBINOMIAL) {
      ctx->err = std::string("AGP_FLAG_SAMPLED: ") + supported() +
                 " (Laplace, BayesianSVM, Poisson, Heteroscedastic, LogisticSoftMax and multi-output models are not sampled yet)";
      return AGP_ERR_UNSUPPORTED;
    }
    if (lp.kind == AGP_LIK_NEGBINOMIAL && desc.lik.p0 != std::floor(desc.lik.p0)) {  // Int(l.r), negativebinomial.jl:87
      ctx->err = "InexactError: the Gibbs sampler of NegBinomialLikelihood(r) draws PolyaGamma(y + Int(r), |f|): r must be an integer";
      return AGP_ERR_INVALID;
    }
    return AGP_OK;
  }
  agp_status init() override {
    AGPCHK(Vgp::init());
    HIPCHK(ctx, hipMemsetAsync(lat[0].mu, 0, sizeof(T) * mp, st()));  // f = 0
    return AGP_OK;
  }
  agp_status sampled_refused(const char* what) {
    ctx->err = std::string("Gibbs-sampled model (AGP_FLAG_SAMPLED): ") + what +
               " is not supported (the chain is advanced by agp_svgp_gibbs_sample and read by agp_svgp_predict_samples; "
               "objective(::MCGP) = NaN and the reference never tunes its kernel)";
    return AGP_ERR_UNSUPPORTED;
  }
  agp_status step_local(const void*, int64_t, const void*, const int64_t*, int64_t, double, bool) override {
    return sampled_refused("agp_svgp_cavi_step");
  }
  agp_status elbo(const void*, int64_t, const void*, const int64_t*, int64_t, double, int, double*) override {
    return sampled_refused("agp_svgp_elbo");
  }
  agp_status elbo_enqueue(const void*, int64_t, const void*, const int64_t*, int64_t, double, int, int32_t*) override {
    return sampled_refused("agp_svgp_elbo_enqueue");
  }
  agp_status elbo_terms(double*) override { return sampled_refused("agp_svgp_elbo_terms"); }
  agp_status hypergrad(int, double*, double*, void*) override { return sampled_refused("agp_svgp_hypergrad"); }
  agp_status hyper_step() override { return sampled_refused("agp_svgp_hyper_step"); }
  agp_status hyper_apply(int, const double*, const double*, const void*) override { return sampled_refused("agp_svgp_hyper_apply"); }
  agp_status hyper_configure(int, double, int, double, double, double, double) override {
    return sampled_refused("agp_svgp_hyper_configure");
  }
  agp_status hyper_rule(int, double, int, double) override { return sampled_refused("agp_svgp_hyper_rule"); }
  agp_status pathwise_draw(int, int, uint64_t, int64_t, agp_pathwise**) override {
    return pathwise_refused("Gibbs-sampled models (AGP_FLAG_SAMPLED) are not supported: their samples are read by "
                            "agp_svgp_predict_samples");
  }
  agp_status predict_f(const void*, int64_t, int64_t, void*, void*) override { return sampled_refused("agp_svgp_predict_f"); }
  agp_status predict_f_cov(const void*, int64_t, int64_t, void*, void*) override { return sampled_refused("agp_svgp_predict_f_cov"); }
  agp_status predict_y(const void*, int64_t, int64_t, void*) override { return sampled_refused("agp_svgp_predict_y"); }
  agp_status proba_y(const void*, int64_t, int64_t, const double*, const double*, int, void*, void*) override {
    return sampled_refused("agp_svgp_proba_y");
  }

  // one sweep at counter gibbs_t (AbstractMCMC.step, sampling.jl:36-75); keep: the sweep's row of the caller's store, or NULL
  agp_status sweep(const T* y, uint64_t seed, T* keep) {
    Latent& g = lat[0];
    const uint32_t t = (uint32_t)gibbs_t;
    int ns = 0;
    AGPCHK(colstats_part(&ns));
    hipLaunchKernelGGL((k_gibbs_local<T>), grid1(m), dim3(256), 0, st(), m, lp, y, (const T*)g.mu, seed, t, theta, cbuf, rbuf, wbuf,
                       flags_dev);
    hipLaunchKernelGGL((k_vgp_eta<T>), dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, st(), m, mp,
                       (const T*)kinv_step(g), (const T*)rbuf, (const T*)wbuf, (const T*)kinv_mu0_step(g), g.eta2, g.La, g.eta1);
    LAUNCHCHK(ctx);
    g.la_state = 0;
    g.xa_valid = false;
    AGPCHK(vgp_factor(g));
    const int64_t ntc = mp / TILE, rows = (mp + ns - 1) / ns;
    hipLaunchKernelGGL((k_gibbs_f<T>), dim3((unsigned)ntc, (unsigned)ns), dim3(256), 0, st(), m, mp, (const T*)g.Xa, (const T*)g.v,
                       rows, seed, t, vgp_part, flags_dev);
    hipLaunchKernelGGL((k_gibbs_fsum<T>), grid1(m), dim3(256), 0, st(), m, mp, ns, (const T*)vgp_part, g.mu, keep);
    LAUNCHCHK(ctx);
    gibbs_t += 1;
    swept = true;
    return AGP_OK;
  }
  agp_status gibbs_sample(const void* y, int64_t n_samples, int64_t discard_initial, int64_t thinning, uint64_t seed, void* store,
                          int64_t lds) override {
    if (!y || !store || n_samples < 1 || discard_initial < 0 || thinning < 1 || lds < m) {
      ctx->err = "agp_svgp_gibbs_sample: y and store must be given, n_samples >= 1, discard_initial >= 0, thinning >= 1, lds >= N";
      return AGP_ERR_INVALID;
    }
    const int64_t total = discard_initial + 1 + (n_samples - 1) * thinning;
    if (gibbs_t + total > (int64_t)0xFFFFFFFFll) {
      ctx->err = "agp_svgp_gibbs_sample: the sweep counter is one 32-bit word of the generator's counter";
      return AGP_ERR_INVALID;
    }
    AGPCHK(refresh_K());
    for (int64_t s = 1; s <= total; ++s) {
      const int64_t k = s - discard_initial - 1;
      const bool kept = k >= 0 && k % thinning == 0;
      AGPCHK(sweep((const T*)y, seed, kept ? (T*)store + (k / thinning) * lds : (T*)nullptr));
    }
    record_batch(y, 1.0);
    return AGP_OK;
  }
  agp_status gibbs_counter(int set, int64_t* t) override {
    if (!t) return AGP_ERR_INVALID;
    if (set) {
      if (*t < 0 || *t > (int64_t)0xFFFFFFFFll) return AGP_ERR_INVALID;
      gibbs_t = *t;
    } else {
      *t = gibbs_t;
    }
    return AGP_OK;
  }
  // mu <- f, sigma <- Sigma = inv(2 Diagonal(grad_E_Sigma) + inv(K)) of the last sweep (I before the first); no natural parameters
  agp_status get_state(int l, void* mu, void* sigma, void* eta1, void* eta2) override {
    if (l != 0) return AGP_ERR_INVALID;
    if (eta1 || eta2) {
      ctx->err = "Gibbs-sampled model (AGP_FLAG_SAMPLED): the state is a sample, not a variational posterior (eta1 / eta2 must be NULL)";
      return AGP_ERR_UNSUPPORTED;
    }
    Latent& g = lat[0];
    if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, g.mu, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    if (sigma) {
      if (swept)
        AGPCHK(xtx_padded<T>(ctx, g.Xa, mp, mp, g.Sigma, mp));
      else
        hipLaunchKernelGGL((k_set_identity<T>), grid2(mp, mp), blk2, 0, st(), g.Sigma, mp, mp, T(1));
      LAUNCHCHK(ctx);
      HIPCHK(ctx, hipMemcpy2DAsync(sigma, sizeof(T) * m, g.Sigma, sizeof(T) * mp, sizeof(T) * m, m, hipMemcpyDeviceToDevice, st()));
    }
    return AGP_OK;
  }
  // installs f, the state the chain continues from (eta1 = f, eta2 = NULL): what a reloaded model needs next to the sweep counter
  agp_status set_state(int l, const void* f, const void* eta2) override {
    if (l != 0 || !f) return AGP_ERR_INVALID;
    if (eta2) {
      ctx->err = "Gibbs-sampled model (AGP_FLAG_SAMPLED): set_state installs f (eta1 = f); eta2 must be NULL";
      return AGP_ERR_UNSUPPORTED;
    }
    HIPCHK(ctx, hipMemcpyAsync(lat[0].mu, f, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }

  // _predict_f(::MCGP) / proba_y(::MCGP) (predictions.jl:94-130, 260-276): F* = K*n (K \ F) for all kept samples, block of test
  // points by block (K*n is never held whole), then mean / variance over the samples per test point (k_mcgp_pred_finish)
  agp_status predict_samples(const void* xt, int64_t ldx, int64_t nt, const void* store, int64_t lds, int64_t S, int mode,
                             void* out0, void* out1) override {
    if (!xt || nt <= 0 || ldx < D || !store || lds < m || S < 1 || !out0 || mode < 0 || mode > 2 || (mode != 0 && !out1)) {
      ctx->err = "agp_svgp_predict_samples: xt, store and out0 must be given (out1 too unless mode = 0), n_t > 0, ldx >= D, lds >= N, "
                 "n_samples >= 1, mode 0, 1 or 2";
      return AGP_ERR_INVALID;
    }
    if (S > MC_MAX_SAMPLES) {
      ctx->err = "agp_svgp_predict_samples: at most " + std::to_string(MC_MAX_SAMPLES) + " samples per call (got " +
                 std::to_string(S) + "): thin the store or predict from a part of it";
      return AGP_ERR_INVALID;
    }
    if (mode == 2 && lp.kind != AGP_LIK_LOGISTIC) {
      ctx->err = "agp_svgp_predict_samples: mode 2 (mean and variance of logistic(f*) over the samples) is proba_y of the Bernoulli "
                 "likelihood (predictions.jl:266-276); other likelihoods take compute_proba on the moments of mode 1";
      return AGP_ERR_UNSUPPORTED;
    }
    Latent& g = lat[0];
    AGPCHK(params_to_host(g));
    AGPCHK(ensure_pred_ws(0, true));
    AGPCHK(refresh_K());
    AGPCHK(ensure_zsc(g));
    const int64_t Sp = rup64(S), CH = pred_chunk;
    if (Sp > mc_sp) {
      for (T** p : {&mc_Fs, &mc_G, &mc_Fstar}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
      }
      mc_sp = 0;
      AGPCHK(dmalloc(ctx, &mc_Fs, Sp * mp));
      AGPCHK(dmalloc(ctx, &mc_G, Sp * mp));
      AGPCHK(dmalloc(ctx, &mc_Fstar, CH * Sp));
      mc_sp = Sp;
    }
    HIPCHK(ctx, hipMemsetAsync(mc_Fs, 0, sizeof(T) * mc_sp * mp, st()));
    HIPCHK(ctx, hipMemcpy2DAsync(mc_Fs, sizeof(T) * mp, store, sizeof(T) * lds, sizeof(T) * m, S, hipMemcpyDeviceToDevice, st()));
    // G = F K^-1 (rows = samples; K^-1 symmetric)
    AGPCHK((gemm_nt<T, EPI_STORE>(ctx, mc_Fs, mp, g.Kinv, mp, Sp, mp, mp, 0, mc_G, mp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
    for (int64_t s = 0; s < nt; s += CH) {
      const int64_t nc = (nt - s) < CH ? (nt - s) : CH, nq = rup64(nc);
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)xt + s * ldx, ldx, (const int64_t*)nullptr, nc, (const T*)g.Z, D, m, D,
                                   (const T*)g.scales, g.k.kind, kvar(g), Kstar, mp, nq, mp, 0, T(0), (const T*)nullptr, (T*)nullptr,
                                   (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, Kstar, mp, mc_G, mp, nq, Sp, mp, 0, mc_Fstar, Sp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      if (mode == 1)
        AGPCHK((gemm_nt<T, EPI_ROWDOT>(ctx, Kstar, mp, g.Kinv, mp, nq, mp, mp, 0, nullptr, 0, Kstar, mp, nullptr, ppv, nullptr, CH)));
      hipLaunchKernelGGL((k_mcgp_pred_finish<T>), grid1(nc), dim3(256), 0, st(), nc, (int)S, (const T*)mc_Fstar, Sp, mode,
                         (int)(2 * mp / TILE), (const T*)ppv, CH, (T)g.k.variance, (T)jitter, (T*)out0 + s,
                         out1 ? (T*)out1 + s : (T*)nullptr);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }
};

// ---- numerical inference on the full model (AGP_FLAG_FULL | AGP_FLAG_NUMERICAL: VGP(X, y, kernel, likelihood, QuadratureVI())) ----
// src/inference/numericalVI.jl, src/inference/quadratureVI.jl.  The state is (mu, Sigma) itself -- kept in g.mu / g.Sigma with
// g.post_valid always set, so predictions read it where materialize() would have left it -- and the optimiser moments of both.
// One step (nvi_step): k_vgp_diag + k_quad_local give g, h at the current posterior; k_nvi_grad_mu forms the gradient of eta1 and
// the rule's d mu; the gradient of eta2 is, in natural mode, (Sigma Diagonal(h) - Sigma K^-1) Sigma + Sigma (two gemm_nt, no inverse of
// Sigma), in classical mode Diagonal(h / 2) - (K^-1 - Sigma^-1) / 2 with Sigma^-1 from the inverse factor of the accepted Sigma;
// k_nvi_grad_sigma applies the rule on the upper triangle and mirrors it; the backtracking forms Sigma + alpha D (k_nvi_candidate),
// factors it (potrf_fused) and reads the pivot status on the HOST once per attempt.  The accepted factor stays in nv_F / nv_Dg
// (log det Sigma of the ELBO) and nv_X (its inverse, classical mode).
static double nvi_lconst(int kind, double p0) {
  if (kind == AGP_LIK_STUDENTT)  // studentt.jl:43-46 as written: Gamma(alpha) / (sqrt(nu pi) Gamma(nu / 2)), alpha = (nu + 1) / 2
    return std::lgamma(0.5 * (p0 + 1.0)) - 0.5 * std::log(p0 * 3.141592653589793) - std::lgamma(0.5 * p0);
  if (kind == AGP_LIK_LAPLACE) return -std::log(2.0 * p0);
  return 0.0;
}
static bool nvi_lik_ok(int kind) { return kind == AGP_LIK_LOGISTIC || kind == AGP_LIK_STUDENTT || kind == AGP_LIK_LAPLACE; }
static const char* nvi_supported() {
  return "quadrature inference on the device runs for the Logistic, StudentT and Laplace likelihoods, Float64, one latent, on the "
         "full model (AGP_FLAG_FULL | AGP_FLAG_NUMERICAL) and the sparse model (AGP_FLAG_NUMERICAL)";
}
// Monte-Carlo inference (AGP_FLAG_MC on top of AGP_FLAG_NUMERICAL: MCIntegrationVI / MCIntegrationSVI, src/inference/MCVI.jl)
static bool mc_lik_ok(int kind) { return kind == AGP_LIK_SOFTMAX || kind == AGP_LIK_LOGISTICSOFTMAX; }
static const char* mc_supported() {
  return "Monte-Carlo inference on the device runs for the SoftMax and LogisticSoftMax likelihoods, Float64, n_latent = n_class = K "
         "with 2 <= K <= 64, on the full model (AGP_FLAG_FULL | AGP_FLAG_NUMERICAL | AGP_FLAG_MC) and the sparse model "
         "(AGP_FLAG_NUMERICAL | AGP_FLAG_MC)";
}
// the table eps[nMC][K] of (seed, t, stream) (agp_rand.h)
static agp_status mc_fill_normals(agp_ctx* ctx, hipStream_t s, uint64_t seed, int64_t t, int stream, int nMC, int K, double* out) {
  const int64_t n = (int64_t)nMC * K;
  hipLaunchKernelGGL(k_mc_normals, grid1(n), dim3(256), 0, s, n, seed, (uint32_t)t, (uint32_t)stream, out);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

struct Nvgp : Vgp {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("numerical inference on the full model (AGP_FLAG_NUMERICAL / AGP_FLAG_MC with AGP_FLAG_FULL) is not supported");
  }
  agp_status pathwise_draw(int, int, uint64_t, int64_t, agp_pathwise**) override {
    return pathwise_refused("numerical inference (AGP_FLAG_NUMERICAL, with or without AGP_FLAG_MC) is not supported yet -- a "
                            "follow-up: the factor of Sigma is already kept on such a handle");
  }
  bool configured = false, natural = true;
  int nn = 0;
  NviRule rule{};
  double* quad_dev = nullptr;  // [nodes | weights]
  int64_t nv_t = 0;            // steps taken: ADAM's t of both states of every latent, and t of the Monte-Carlo streams
  // what every latent keeps of its own: K + jitt I unfactored, the accepted factor of Sigma (F, diagonal tiles Dg, inverse X), the
  // optimiser's moments, and the backtracking's record.  12 m x m matrices per latent with those of the base handle.
  struct NvLat {
    T *K = nullptr, *F = nullptr, *X = nullptr, *Dg = nullptr;
    double *mom_mu = nullptr, *mom_S = nullptr;  // [2][mp], [2][mp][mp]: Momentum's vel / ADAM's m, then ADAM's v
    double alpha_last = 1.0;
    int64_t halvings_total = 0, rejected_total = 0;
    bool factor_valid = false, K_valid = false;
  };
  std::vector<NvLat> nvl;
  int cur = 0;  // the latent that update_from / factor_candidate / ensure_factor work on
  T *nv_A = nullptr, *nv_D = nullptr, *nv_C = nullptr, *nv_dmu = nullptr;  // scratch, one latent at a time
  int32_t* nv_info = nullptr;
  bool mc = false;  // AGP_FLAG_MC: the expectations by Monte-Carlo integration over K latents
  int nMC = 0;
  uint64_t mc_seed = 0;
  double* mc_eps = nullptr;  // [nMC][K], refilled for every step and every ELBO evaluation
  ~Nvgp() override {
    for (auto& q : nvl) {
      for (T* p : {q.K, q.F, q.X, q.Dg})
        if (p) dfree(p);
      for (double* p : {q.mom_mu, q.mom_S})
        if (p) dfree(p);
    }
    for (T* p : {nv_A, nv_D, nv_C, nv_dmu})
      if (p) dfree(p);
    for (double* p : {quad_dev, mc_eps})
      if (p) dfree(p);
    if (nv_info) dfree(nv_info);
  }
  // AGP_FLAG_MC: judged on the descriptor itself, before the checks of the analytic handle
  agp_status mc_check_desc() {
    mc = (desc.flags & AGP_FLAG_MC) != 0;
    if (!mc) return AGP_OK;
    if (!mc_lik_ok(desc.lik.kind) || desc.n_latent < 2 || desc.n_latent > MC_KMAX || desc.lik.n_class != desc.n_latent ||
        desc.latent_offset != 0) {
      ctx->err = std::string("AGP_FLAG_MC: ") + mc_supported();
      return AGP_ERR_UNSUPPORTED;
    }
    return AGP_OK;
  }
  agp_status lik_check() {
    if (mc) return AGP_OK;
    if (lp.kind == AGP_LIK_GAUSSIAN) {  // test/likelihood/gaussian.jl:38,59
      ctx->err = "The GaussianLikelihood is not compatible with QuadratureVI: use AnalyticVI (the expectations are closed-form)";
      return AGP_ERR_UNSUPPORTED;
    }
    if (!nvi_lik_ok(lp.kind) || nl != 1) {
      ctx->err = std::string("AGP_FLAG_NUMERICAL: ") + nvi_supported();
      return AGP_ERR_UNSUPPORTED;
    }
    return AGP_OK;
  }
  agp_status check_desc() override {
    AGPCHK(mc_check_desc());
    AGPCHK(Svgp<T>::check_desc());
    AGPCHK(check_full());
    return lik_check();
  }
  agp_status init() override {
    AGPCHK(Vgp::init());
    const int64_t mm = mp * mp;
    nvl.resize(nl);
    for (auto& q : nvl) {
      for (T** p : {&q.K, &q.F, &q.X}) AGPCHK(dmalloc(ctx, p, mm));
      AGPCHK(dmalloc(ctx, &q.Dg, mp * TILE));
      AGPCHK(dmalloc(ctx, &q.mom_mu, 2 * mp));
      AGPCHK(dmalloc(ctx, &q.mom_S, 2 * mm));
    }
    for (T** p : {&nv_A, &nv_D, &nv_C}) AGPCHK(dmalloc(ctx, p, mm));
    AGPCHK(dmalloc(ctx, &nv_dmu, mp));
    AGPCHK(dmalloc(ctx, &nv_info, 1));
    for (auto& g : lat) {
      HIPCHK(ctx, hipMemsetAsync(g.mu, 0, sizeof(T) * mp, st()));  // VarPosterior{T}(dim): mu = 0, Sigma = I (posterior.jl:29-37)
      hipLaunchKernelGGL((k_set_identity<T>), grid2(mp, mp), blk2, 0, st(), g.Sigma, mp, mp, T(1));
      LAUNCHCHK(ctx);
      g.post_valid = true;
    }
    return zero_moments();
  }
  agp_status zero_moments() {
    for (auto& q : nvl) {
      HIPCHK(ctx, hipMemsetAsync(q.mom_mu, 0, sizeof(double) * 2 * mp, st()));
      HIPCHK(ctx, hipMemsetAsync(q.mom_S, 0, sizeof(double) * 2 * mp * mp, st()));
    }
    nv_t = 0;
    return AGP_OK;
  }
  agp_status numerical_refused(const char* what) {
    ctx->err = std::string("numerical inference (AGP_FLAG_NUMERICAL): ") + what +
               " is not supported (the posterior moves by agp_svgp_nvi_step; the hyper-parameter step through the quadrature ELBO "
               "is not built)";
    return AGP_ERR_UNSUPPORTED;
  }
  agp_status step_local(const void*, int64_t, const void*, const int64_t*, int64_t, double, bool) override {
    return numerical_refused("agp_svgp_cavi_step");
  }
  agp_status hypergrad(int, double*, double*, void*) override { return numerical_refused("agp_svgp_hypergrad"); }
  agp_status hyper_step() override { return numerical_refused("agp_svgp_hyper_step"); }
  agp_status hyper_apply(int, const double*, const double*, const void*) override { return numerical_refused("agp_svgp_hyper_apply"); }
  agp_status hyper_configure(int, double, int, double, double, double, double) override {
    return numerical_refused("agp_svgp_hyper_configure");
  }
  agp_status hyper_rule(int, double, int, double) override { return numerical_refused("agp_svgp_hyper_rule"); }

  // the optimiser's part of agp_svgp_nvi_configure and agp_svgp_mcvi_configure
  agp_status check_rule(const char* what, int opt_kind, double eta, double p1, double p2, double eps) {
    if ((opt_kind == AGP_OPT_MOMENTUM && !(p1 >= 0 && p1 < 1)) ||
        (opt_kind == AGP_OPT_ADAM && !(p1 >= 0 && p1 < 1 && p2 >= 0 && p2 < 1 && eps >= 0))) {
      ctx->err = std::string(what) + ": Momentum takes 0 <= rho < 1 (p1), ADAM 0 <= beta1, beta2 < 1 (p1, p2) and eps >= 0";
      return AGP_ERR_INVALID;
    }
    return AGP_OK;
  }
  void install_rule(int nat, int opt_kind, double eta, double p1, double p2, double eps) {
    if (natural != (nat != 0))
      for (auto& q : nvl) q.factor_valid = false;  // classical mode keeps the inverse factor as well
    natural = nat != 0;
    rule.kind = opt_kind;
    rule.eta = eta;
    rule.p1 = p1;
    rule.p2 = p2;
    rule.eps = eps;
    rule.c1 = rule.c2 = 1.0;
    configured = true;
  }
  agp_status nvi_configure(int n, const double* nodes, const double* weights, int nat, int opt_kind, double eta, double p1,
                           double p2, double eps) override {
    if (mc) {
      ctx->err = "agp_svgp_nvi_configure: the handle runs Monte-Carlo integration (AGP_FLAG_MC); configure it with "
                 "agp_svgp_mcvi_configure";
      return AGP_ERR_UNSUPPORTED;
    }
    if (n < 1 || n > 4096 || !nodes || !weights || !(eta > 0) ||
        (opt_kind != AGP_OPT_ADAM && opt_kind != AGP_OPT_DESCENT && opt_kind != AGP_OPT_MOMENTUM)) {
      ctx->err = "agp_svgp_nvi_configure: 1 <= n <= 4096 nodes and weights, eta > 0, opt_kind one of AGP_OPT_ADAM / DESCENT / MOMENTUM";
      return AGP_ERR_INVALID;
    }
    AGPCHK(check_rule("agp_svgp_nvi_configure", opt_kind, eta, p1, p2, eps));
    if (n != nn) {
      if (quad_dev) dfree(quad_dev);
      quad_dev = nullptr;
      nn = 0;
      AGPCHK(dmalloc(ctx, &quad_dev, 2 * (int64_t)n));
      nn = n;
    }
    HIPCHK(ctx, hipMemcpyAsync(quad_dev, nodes, sizeof(double) * n, hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipMemcpyAsync(quad_dev + n, weights, sizeof(double) * n, hipMemcpyHostToDevice, st()));
    HIPCHK(ctx, hipStreamSynchronize(st()));  // (the caller's arrays may go away)
    install_rule(nat, opt_kind, eta, p1, p2, eps);
    return AGP_OK;
  }
  agp_status mcvi_configure(int n, uint64_t seed, int nat, int opt_kind, double eta, double p1, double p2, double eps) override {
    if (!mc) {
      ctx->err = "agp_svgp_mcvi_configure: the handle runs quadrature (no AGP_FLAG_MC); configure it with agp_svgp_nvi_configure";
      return AGP_ERR_UNSUPPORTED;
    }
    if (n < 1 || n > 65536 || !(eta > 0) ||
        (opt_kind != AGP_OPT_ADAM && opt_kind != AGP_OPT_DESCENT && opt_kind != AGP_OPT_MOMENTUM)) {
      ctx->err = "agp_svgp_mcvi_configure: 1 <= nMC <= 65536, eta > 0, opt_kind one of AGP_OPT_ADAM / DESCENT / MOMENTUM";
      return AGP_ERR_INVALID;
    }
    AGPCHK(check_rule("agp_svgp_mcvi_configure", opt_kind, eta, p1, p2, eps));
    if (n != nMC) {
      if (mc_eps) dfree(mc_eps);
      mc_eps = nullptr;
      nMC = 0;
      AGPCHK(dmalloc(ctx, &mc_eps, (int64_t)n * nl));
      nMC = n;
    }
    mc_seed = seed;
    install_rule(nat, opt_kind, eta, p1, p2, eps);
    return AGP_OK;
  }
  agp_status need_config(const char* what) {
    if (configured) return AGP_OK;
    ctx->err = std::string(what) + (mc ? ": install nMC, the seed and the optimiser first (agp_svgp_mcvi_configure)"
                                       : ": install the quadrature rule and the optimiser first (agp_svgp_nvi_configure)");
    return AGP_ERR_INVALID;
  }
  agp_status check_latent(int l) { return l >= 0 && l < nl ? AGP_OK : AGP_ERR_INVALID; }
  // K + jitt I unfactored (the natural gradient of eta1 multiplies by it) next to the factor, inverse and log det of refresh_K
  agp_status ensure_K() {
    std::vector<char> stale(nl);
    for (int l = 0; l < nl; ++l) stale[l] = lat[l].K_stale ? 1 : 0;
    AGPCHK(refresh_K());
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      NvLat& q = nvl[l];
      if (stale[l] || !q.K_valid) {
        AGPCHK(ensure_zsc(g));
        (void)launch_kernelmatrix<T>(ctx, st(), (const T*)g.Z, D, (const int64_t*)nullptr, m, (const T*)g.Z, D, m, D,
                                     (const T*)g.scales, g.k.kind, kvar(g), q.K, mp, mp, mp, 1, (T)jitter, (const T*)nullptr, (T*)nullptr,
                                     (int64_t)0, 0, (const T*)g.Zsc, (const T*)g.zn);
        LAUNCHCHK(ctx);
        q.K_valid = true;
      }
    }
    return AGP_OK;
  }
  // factor Sigma + alpha D of the current latent (F, diagonal tiles Dg; with its inverse X in classical mode); *info: 0, or the
  // leading minor that is not positive.  Sigma + alpha D itself is left in nv_C (keep_c).
  agp_status factor_candidate(const T* Dm, T alpha, bool keep_c, int32_t* info) {
    Latent& g = lat[cur];
    NvLat& q = nvl[cur];
    const int do_x = natural ? 0 : 1;
    for (int pass = 0; pass < 2; ++pass) {
      HIPCHK(ctx, hipMemsetAsync(nv_info, 0, sizeof(int32_t), st()));
      hipLaunchKernelGGL((k_nvi_candidate<T>), grid2(mp, mp), blk2, 0, st(), m, mp, mp, (const T*)g.Sigma, Dm, alpha,
                         keep_c ? nv_C : (T*)nullptr, q.F);
      LAUNCHCHK(ctx);
      PotrfReq<T> rq{};
      rq.A = q.F, rq.ld = mp, rq.n = mp, rq.X = q.X, rq.ldx = mp, rq.Dg = q.Dg, rq.do_x = do_x, rq.info_dev = nv_info, rq.nvalid = m;
      AGPCHK(potrf_fused<T>(ctx, rq));
      HIPCHK(ctx, hipMemcpyAsync(info, nv_info, sizeof(int32_t), hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      if (*info != -1 || pass == 1) break;
      bool lost = false;  // the task graph lost a tile dependency: plain launches from here on, the candidate is formed again
      AGPCHK(dag_lost_dependency(ctx, nv_info, &lost));
      if (!lost) break;
    }
    if (*info < 0) {
      ctx->err = "numerical inference: the factorisation of Sigma + alpha dSigma aborted (a tile dependency never arrived)";
      return AGP_ERR_HIP;
    }
    return AGP_OK;
  }
  agp_status ensure_factor() {
    NvLat& q = nvl[cur];
    if (q.factor_valid) return AGP_OK;
    int32_t info = 0;
    AGPCHK(factor_candidate((const T*)lat[cur].Sigma, T(0), false, &info));
    if (info != 0) {
      ctx->err = "PosDefException: Sigma is not positive definite; leading minor " + std::to_string(info);
      return AGP_ERR_NOT_POSDEF;
    }
    q.factor_valid = true;
    return AGP_OK;
  }
  agp_status ensure_factors() {
    for (cur = 0; cur < nl; ++cur) AGPCHK(ensure_factor());
    cur = 0;
    return AGP_OK;
  }
  agp_status check_whole_set(const void* y, const int64_t* idx, int64_t B) {
    if (idx != nullptr || B != m) {
      ctx->err = "full model (AGP_FLAG_FULL): steps and ELBO evaluations run on the whole training set (idx = NULL, B = N = m)";
      return AGP_ERR_BAD_BATCH;
    }
    if (!y) {
      ctx->err = "numerical inference: y must be given";
      return AGP_ERR_INVALID;
    }
    return AGP_OK;
  }
  void quad_local(int64_t B, const T* y, const int64_t* idx, const T* mf, const T* vf, T* ell, T* gq, T* hq) {
    hipLaunchKernelGGL((k_quad_local<T>), grid1(B), dim3(256), 0, st(), B, lp, nvi_lconst(lp.kind, desc.lik.p0), y, idx, mf, vf,
                       (const double*)quad_dev, (const double*)(quad_dev + nn), nn, ell, gq, hq);
  }
  // ell [B], g and h [nl][Bp] of the batch from its moments mf, vf [nl][Bp]: the quadrature for the single latent, or the
  // Monte-Carlo table of stream 2 at step nv_t + 1 (a step) / stream 3 at nv_t (an ELBO evaluation) over the K latents
  agp_status local_expectations(int64_t B, const void* y, const int64_t* idx, const T* mf, const T* vf, T* ell, T* gq, T* hq,
                                bool for_elbo) {
    if (!mc) {
      quad_local(B, (const T*)y, idx, mf, vf, ell, gq, hq);
      return AGP_OK;
    }
    const int64_t t = for_elbo ? nv_t : nv_t + 1;
    if (t > (int64_t)0xFFFFFFFFll) {
      ctx->err = "Monte-Carlo inference: the step counter must stay below 2^32";
      return AGP_ERR_INVALID;
    }
    AGPCHK(mc_fill_normals(ctx, st(), mc_seed, t, for_elbo ? RNG_STREAM_MC_ELBO : RNG_STREAM_MC_GRAD, nMC, nl, mc_eps));
    hipLaunchKernelGGL(k_mc_local, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st(), B, (int)lp.kind, nl, nMC, (const int32_t*)y, idx,
                       (const double*)mf, (const double*)vf, Bp, (const double*)mc_eps, (double*)ell, (double*)gq, (double*)hq, Bp,
                       flags_dev);
    return AGP_OK;
  }

  // variational_updates + global_update! (numericalVI.jl:101-179) for every latent; rho = 1 on the full model
  agp_status nvi_step(const void*, int64_t, const void* y, const int64_t* idx, int64_t B, double rho) override {
    AGPCHK(need_config("agp_svgp_nvi_step"));
    AGPCHK(check_whole_set(y, idx, B));
    if (rho != 1.0) {
      ctx->err = "agp_svgp_nvi_step: the full model takes rho = 1";
      return AGP_ERR_INVALID;
    }
    AGPCHK(ensure_K());
    if (!natural) AGPCHK(ensure_factors());
    for (int l = 0; l < nl; ++l)
      hipLaunchKernelGGL((k_vgp_diag<T>), grid1(m), dim3(256), 0, st(), m, mp, (const T*)lat[l].Sigma, (const T*)lat[l].mu, muf + l * Bp,
                         varf + l * Bp);
    AGPCHK(local_expectations(m, y, nullptr, muf, varf, Kt, rbuf, wbuf, false));
    LAUNCHCHK(ctx);
    for (int l = 0; l < nl; ++l) {
      cur = l;
      AGPCHK(update_from(rbuf + l * Bp, nullptr, wbuf + l * Bp, l == nl - 1));
    }
    cur = 0;
    record_batch(y, 1.0);
    return AGP_OK;
  }
  // the optimiser step on mu and Sigma of the current latent and its backtracking, from u = rho kappa' g (the full model: g), the
  // data term P2 of the gradient of eta2 (sparse model: rho W Diagonal(h) W' or rho kappa' Diagonal(h) kappa, m x m; the full model:
  // NULL) and h (the full model's diagonal data term; NULL with P2).  last: the step's last latent -- the shared counter moves
  agp_status update_from(const T* u, const T* P2, const T* hd, bool last = true) {
    Latent& g = lat[cur];
    NvLat& q = nvl[cur];
    const int64_t t1 = nv_t + 1;  // (the counter moves once every rule has been applied: it never runs ahead of the moments)
    if (rule.kind == AGP_OPT_ADAM) {
      rule.c1 = 1.0 - std::pow(rule.p1, (double)t1);
      rule.c2 = 1.0 - std::pow(rule.p2, (double)t1);
    }
    hipLaunchKernelGGL((k_nvi_grad_mu<T>), grid1(m * 64), dim3(256), 0, st(), m, mp, natural ? 1 : 0,
                       (const T*)(natural ? q.K : g.Kinv), u, (const T*)g.mu, (const T*)g.mu0, rule, q.mom_mu, q.mom_mu + mp, nv_dmu);
    LAUNCHCHK(ctx);
    const int64_t mm = mp * mp;
    if (natural) {
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Sigma, mp, g.Kinv, mp, mp, mp, mp, 0, nv_A, mp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      hipLaunchKernelGGL((k_nvi_left<T>), grid2(mp, mp), blk2, 0, st(), m, mp, mp, (const T*)g.Sigma, hd, nv_A);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, nv_A, mp, g.Sigma, mp, mp, mp, mp, 0, nv_C, mp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      hipLaunchKernelGGL((k_nvi_grad_sigma<T>), grid2(mp, mp), blk2, 0, st(), m, mp, mp, 1, (const T*)nv_C, (const T*)nullptr, P2,
                         (const T*)g.Sigma, hd, rule, q.mom_S, q.mom_S + mm, nv_D);
    } else {
      AGPCHK(xtx_padded<T>(ctx, q.X, mp, mp, nv_A, mp));  // Sigma^-1 from the inverse factor of the accepted Sigma
      hipLaunchKernelGGL((k_nvi_grad_sigma<T>), grid2(mp, mp), blk2, 0, st(), m, mp, mp, 0, (const T*)g.Kinv, (const T*)nv_A, P2,
                         (const T*)g.Sigma, hd, rule, q.mom_S, q.mom_S + mm, nv_D);
    }
    hipLaunchKernelGGL((k_nvi_add<T>), grid1(m), dim3(256), 0, st(), m, g.mu, (const T*)nv_dmu);
    LAUNCHCHK(ctx);
    if (last) nv_t = t1;
    // alpha = 1; while !isposdef(Sigma + alpha Symmetric(dSigma)) && alpha > 1e-8: alpha /= 2; alpha > 1e-8 ? accept : Sigma unchanged
    // (the attempt at the first alpha <= 1e-8 cannot change the outcome and is not made)
    double a = 1.0;
    bool accepted = false;
    q.factor_valid = false;
    while (a > 1e-8) {
      int32_t info = 0;
      AGPCHK(factor_candidate((const T*)nv_D, (T)a, true, &info));
      if (info == 0) {
        accepted = true;
        break;
      }
      a *= 0.5;
      q.halvings_total += 1;
    }
    q.alpha_last = a;
    if (accepted) {
      std::swap(g.Sigma, nv_C);  // the accepted candidate becomes Sigma (both are handle-owned mp x mp buffers: no copy)
      q.factor_valid = true;
    } else {
      q.rejected_total += 1;  // (mu has moved already, numericalVI.jl:166)
    }
    g.pred_valid = g.predvar_valid = false;
    if (tw2_kis_of == cur) tw2_kis_of = -1;
    if (last) n_steps += 1;
    return AGP_OK;
  }
  agp_status nvi_info(int l, double* a_last, int64_t* halvings, int64_t* rejected) override {
    AGPCHK(check_latent(l));
    if (a_last) *a_last = nvl[l].alpha_last;
    if (halvings) *halvings = nvl[l].halvings_total;
    if (rejected) *rejected = nvl[l].rejected_total;
    return AGP_OK;
  }
  // the optimiser moments [2][m] and [2][m][m] of one latent (device, contiguous) and the shared step counter: what a saved model
  // continues from
  agp_status nvi_state(int l, int set, void* mmu, void* msig, int64_t* t) override {
    if (check_latent(l) != AGP_OK || !mmu || !msig || !t) return AGP_ERR_INVALID;
    NvLat& q = nvl[l];
    const int64_t mm = mp * mp;
    for (int s = 0; s < 2; ++s) {
      if (set) {
        if (*t < 0) return AGP_ERR_INVALID;
        HIPCHK(ctx, hipMemcpyAsync(q.mom_mu + s * mp, (const double*)mmu + s * m, sizeof(double) * m, hipMemcpyDeviceToDevice, st()));
        HIPCHK(ctx, hipMemcpy2DAsync(q.mom_S + s * mm, sizeof(double) * mp, (const double*)msig + s * m * m, sizeof(double) * m,
                                     sizeof(double) * m, m, hipMemcpyDeviceToDevice, st()));
      } else {
        HIPCHK(ctx, hipMemcpyAsync((double*)mmu + s * m, q.mom_mu + s * mp, sizeof(double) * m, hipMemcpyDeviceToDevice, st()));
        HIPCHK(ctx, hipMemcpy2DAsync((double*)msig + s * m * m, sizeof(double) * m, q.mom_S + s * mm, sizeof(double) * mp,
                                     sizeof(double) * m, m, hipMemcpyDeviceToDevice, st()));
      }
    }
    if (set) nv_t = *t;
    else *t = nv_t;
    return AGP_OK;
  }
  // mean_f, var_f [nl][Bp] of the batch under the current posterior; the full model: mu and diag Sigma on the whole training set
  virtual agp_status batch_moments(const void*, int64_t, const void* y, const int64_t* idx, int64_t B, T* mf, T* vf) {
    AGPCHK(check_whole_set(y, idx, B));
    for (int l = 0; l < nl; ++l)
      hipLaunchKernelGGL((k_vgp_diag<T>), grid1(m), dim3(256), 0, st(), m, mp, (const T*)lat[l].Sigma, (const T*)lat[l].mu, mf + l * Bp,
                         vf + l * Bp);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  // ELBO = rho sum_i ell_i - sum over the latents of GaussianKL at the current posterior (numericalVI.jl:193-206); there are no local
  // variables, so fresh_local changes nothing
  agp_status elbo(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho, int, double* out) override {
    if (!out) return AGP_ERR_INVALID;
    AGPCHK(need_config("agp_svgp_elbo"));
    AGPCHK(ensure_K());
    AGPCHK(ensure_factors());
    AGPCHK(batch_moments(x, ldx, y, idx, B, emuf, evarf));
    AGPCHK(local_expectations(B, y, idx, emuf, evarf, theta, rbuf2, wbuf2, true));
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(1024), 0, st(), (const double*)theta, B, scal_dev);
    double kl = 0.0;
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      hipLaunchKernelGGL((k_logdiag_sum<T>), dim3(1), dim3(1024), 0, st(), (const T*)nvl[l].Dg, m, scal_dev + 2);
      LAUNCHCHK(ctx);
      AGPCHK(frob_dot((const T*)g.Kinv, (const T*)g.Sigma, mp, m, scal_dev + 3));
      hipLaunchKernelGGL((k_axpby<T>), grid1(mp), dim3(256), 0, st(), mp, T(1), (const T*)g.mu, T(-1), (const T*)g.mu0, tmpv);
      hipLaunchKernelGGL((k_trmv_lower<T>), grid1(mp * 64), dim3(256), 0, st(), (const T*)g.Xk, mp, mp, (const T*)tmpv, pw0);
      hipLaunchKernelGGL((k_sumsq<T>), dim3(1), dim3(1024), 0, st(), (const T*)pw0, mp, scal_dev + 4);
      LAUNCHCHK(ctx);
      double h[5];
      HIPCHK(ctx, hipMemcpyAsync(h, scal_dev, sizeof(double) * 5, hipMemcpyDeviceToHost, st()));
      HIPCHK(ctx, hipStreamSynchronize(st()));
      AGPCHK(resolve_logdet(g));
      e_data = h[0];
      kl += 0.5 * (2.0 * g.half_logdetK - 2.0 * h[2] + h[3] + h[4] - (double)m);
    }
    kl_aug = 0.0;
    kl_gauss_last = kl;
    *out = rho * e_data - kl_gauss_last;
    return AGP_OK;
  }
  // mu, Sigma of the posterior; there are no natural parameters on this handle
  agp_status get_state(int l, void* mu, void* sigma, void* eta1, void* eta2) override {
    AGPCHK(check_latent(l));
    if (eta1 || eta2) {
      ctx->err = "numerical inference (AGP_FLAG_NUMERICAL): the state is (mu, Sigma) (eta1 / eta2 must be NULL)";
      return AGP_ERR_UNSUPPORTED;
    }
    Latent& g = lat[l];
    if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, g.mu, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    if (sigma)
      HIPCHK(ctx, hipMemcpy2DAsync(sigma, sizeof(T) * m, g.Sigma, sizeof(T) * mp, sizeof(T) * m, m, hipMemcpyDeviceToDevice, st()));
    return AGP_OK;
  }
  // installs (mu, Sigma) (eta1 = mu, eta2 = Sigma: T[m], T[m][m]); Sigma must be positive definite
  agp_status set_state(int l, const void* mu, const void* sigma) override {
    if (check_latent(l) != AGP_OK || !mu || !sigma) return AGP_ERR_INVALID;
    Latent& g = lat[l];
    HIPCHK(ctx, hipMemsetAsync(g.mu, 0, sizeof(T) * mp, st()));
    HIPCHK(ctx, hipMemcpyAsync(g.mu, mu, sizeof(T) * m, hipMemcpyDeviceToDevice, st()));
    hipLaunchKernelGGL((k_copy2d<T>), grid2(mp, mp), blk2, 0, st(), (const T*)sigma, m, m, m, g.Sigma, mp, mp, mp, T(1), T(1));
    LAUNCHCHK(ctx);
    g.pred_valid = g.predvar_valid = false;
    if (tw2_kis_of == l) tw2_kis_of = -1;
    nvl[l].factor_valid = false;
    cur = l;
    const agp_status s = ensure_factor();
    cur = 0;
    return s;
  }
  // init_state(model): new optimiser states (states.jl:50-84); the posterior belongs to the model and is kept
  agp_status init_state() override {
    AGPCHK(Vgp::init_state());
    return zero_moments();
  }
};

// ---- numerical inference on the sparse model (AGP_FLAG_NUMERICAL without AGP_FLAG_FULL: SVGP(kernel, likelihood, QuadratureVI() /
// QuadratureSVI(B), Z), and with AGP_FLAG_MC MCIntegrationVI() / MCIntegrationSVI(B)) -----------------------------------------------
// Nvgp's state, optimiser, backtracking, ELBO tail and predictions on m inducing points; what differs is the batch side.  Per step and
// latent: K_nm (launch_kernelmatrix on x[idx]), kappa = K_nm K^-1 and kappa' = K^-1 K_mn (two gemm_nt; K^-1 is symmetric), Wt = Sigma kappa'
// (m x B), K~, mean_f = kappa mu and var_f = diag(kappa Sigma kappa') + K~ (k_nvi_fstats); the expectations on the batch (all latents
// at once); then per latent u = rho kappa' g (k_nvi_kappat_g) and the data term of the gradient of eta2 as one product
// S Diagonal(rho h) S' with S = Wt (natural) or kappa' (classical) (k_nvi_scale_cols + gemm_nt), then Nvgp::update_from.  kappa' and Wt
// are kept per latent from the moments to the update; the kernel matrices are recomputed every step: nothing is cached between steps
// and there is no look-ahead.
struct Nsvgp : Nvgp {
  agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) override {
    return elbo_stream_refused("numerical inference on the sparse model (AGP_FLAG_NUMERICAL / AGP_FLAG_MC) is not supported");
  }
  T *ns_Knm = nullptr, *ns_kap = nullptr, *ns_S2 = nullptr, *ns_u = nullptr;
  std::vector<T*> ns_kapt, ns_Wt;  // per latent
  T* ns_P2 = nullptr;  // the data term of the gradient of eta2, m x m (a buffer of its own: F holds the kept factor)
  ~Nsvgp() override {
    for (T* p : {ns_Knm, ns_kap, ns_S2, ns_u, ns_P2})
      if (p) dfree(p);
    for (T* p : ns_kapt)
      if (p) dfree(p);
    for (T* p : ns_Wt)
      if (p) dfree(p);
  }
  agp_status check_desc() override {
    AGPCHK(mc_check_desc());
    AGPCHK(Svgp<T>::check_desc());
    if (desc.latent_offset != 0) return AGP_ERR_INVALID;
    return lik_check();
  }
  agp_status init() override {
    AGPCHK(Nvgp::init());
    for (T** p : {&ns_Knm, &ns_kap, &ns_S2}) AGPCHK(dmalloc(ctx, p, Bp * mp));
    ns_kapt.assign(nl, nullptr);
    ns_Wt.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
      AGPCHK(dmalloc(ctx, &ns_kapt[l], Bp * mp));
      AGPCHK(dmalloc(ctx, &ns_Wt[l], Bp * mp));
    }
    AGPCHK(dmalloc(ctx, &ns_u, mp));
    AGPCHK(dmalloc(ctx, &ns_P2, mp * mp));
    return AGP_OK;
  }
  // K_nm, kappa, kappa', Wt of the batch and its mean_f / var_f, latent by latent
  agp_status batch_moments(const void* x, int64_t ldx, const void* y, const int64_t*idx, int64_t B, T* mf, T* vf) override {
    if (!x || !y || ldx < D) {
      ctx->err = "numerical inference on the sparse model: x and y must be given, ldx >= D";
      return AGP_ERR_INVALID;
    }
    AGPCHK(check_batch(B));
    const int64_t Bq = rup64(B);
    for (int l = 0; l < nl; ++l) {
      Latent& g = lat[l];
      AGPCHK(params_to_host(g));
      AGPCHK(ensure_zsc(g));
      (void)launch_kernelmatrix<T>(ctx, st(), (const T*)x, ldx, idx, B, (const T*)g.Z, D, m, D, (const T*)g.scales, g.k.kind, kvar(g),
                                   ns_Knm, mp, Bq, mp, 0, T(0), (const T*)nullptr, (T*)nullptr, (int64_t)0, 0, (const T*)g.Zsc,
                                   (const T*)g.zn);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, ns_Knm, mp, g.Kinv, mp, Bq, mp, mp, 0, ns_kap, mp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Kinv, mp, ns_Knm, mp, mp, Bq, mp, 0, ns_kapt[l], Bp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, g.Sigma, mp, ns_kap, mp, mp, Bq, mp, 0, ns_Wt[l], Bp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      hipLaunchKernelGGL((k_nvi_fstats<T>), grid1(B * 64), dim3(256), 0, st(), B, m, mp, Bp, (const T*)ns_kap, (const T*)ns_Knm,
                         (const T*)ns_Wt[l], (const T*)g.mu, (T)(g.k.variance + jitter), mf + l * Bp, vf + l * Bp);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  }
  agp_status nvi_step(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho) override {
    AGPCHK(need_config("agp_svgp_nvi_step"));
    if (!(rho > 0)) return AGP_ERR_INVALID;
    AGPCHK(ensure_K());
    if (!natural) AGPCHK(ensure_factors());
    AGPCHK(batch_moments(x, ldx, y, idx, B, muf, varf));
    AGPCHK(local_expectations(B, y, idx, muf, varf, Kt, rbuf, wbuf, false));
    const int64_t Bq = rup64(B);
    for (int l = 0; l < nl; ++l) {
      hipLaunchKernelGGL((k_nvi_kappat_g<T>), grid1(mp * 64), dim3(256), 0, st(), m, mp, B, Bp, (const T*)ns_kapt[l],
                         (const T*)(rbuf + l * Bp), (T)rho, ns_u);
      const T* S = natural ? ns_Wt[l] : ns_kapt[l];
      hipLaunchKernelGGL((k_nvi_scale_cols<T>), grid2(mp, Bq), blk2, 0, st(), m, B, mp, Bq, Bp, S, (const T*)(wbuf + l * Bp), (T)rho, ns_S2);
      LAUNCHCHK(ctx);
      AGPCHK((gemm_nt<T, EPI_STORE>(ctx, ns_S2, Bp, S, Bp, mp, mp, Bq, 0, ns_P2, mp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      cur = l;
      AGPCHK(update_from(ns_u, ns_P2, nullptr, l == nl - 1));
    }
    cur = 0;
    x_last = x;
    y_last = y;
    idx_last = idx;
    B_last = B;
    ldx_last = ldx;
    rho_last = rho;
    return AGP_OK;
  }
};

// ================================================================================================================
// C entry points
// ================================================================================================================
extern "C" {

int32_t agp_version(void) { return 200; }  // 2xx: round-2 ABI (agp_comm_*, *_multi, get_matrix capacity, kernel structure flags)

agp_status agp_ctx_create(int32_t device, void* hip_stream, agp_ctx** out) {
  if (!out) return AGP_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return AGP_ERR_HIP;
  {
    DevGuard guard(device);  // touches the device once (creates its primary context) and puts the caller's back
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) return AGP_ERR_HIP;
  }
  agp_ctx* c = new agp_ctx();
  c->device = device;
  c->stream = (hipStream_t)hip_stream;
  *out = c;
  return AGP_OK;
}

agp_status agp_ctx_destroy(agp_ctx* ctx) {
  if (!ctx) return AGP_OK;
  DevGuard guard(ctx->device);
  step_trace_dump(ctx);
  if (ctx->tri_scratch || ctx->dag_flags || ctx->hset[0]) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->dag_flags) (void)hipFree(ctx->dag_flags);
    for (int q = 0; q < 2; ++q)
      if (ctx->hset[q]) (void)hipFree(ctx->hset[q]);
    if (ctx->tri_scratch) (void)hipFree(ctx->tri_scratch);
  }
  if (ctx->kmm_scratch) (void)hipFree(ctx->kmm_scratch);
  if (ctx->bal_ws) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ctx->bal_ws);
  }
  if (ctx->chain_stream) {
    (void)hipStreamSynchronize(ctx->chain_stream);
    (void)hipStreamDestroy(ctx->chain_stream);
  }
  if (ctx->chain_go) (void)hipFree(ctx->chain_go);
  if (ctx->chain_ctr) (void)hipFree(ctx->chain_ctr);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->chol_li) (void)hipFree(ctx->chol_li);
  if (ctx->safe_bar) (void)hipFree(ctx->safe_bar);
  if (ctx->safe_retries) (void)hipFree(ctx->safe_retries);
  delete ctx;
  return AGP_OK;
}

agp_status agp_ctx_sync(agp_ctx* ctx) {
  if (!ctx) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

// task-graph launches of this context that lost a tile dependency and were re-run by the in-stream fallback (cumulative)
agp_status agp_ctx_task_graph_fallbacks(agp_ctx* ctx, int64_t* n_host) {
  if (!ctx || !n_host) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  *n_host = 0;
  if (!ctx->safe_retries) return AGP_OK;  // no launch of this context ever carried a fallback
  int32_t r = 0;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(&r, ctx->safe_retries, sizeof(r), hipMemcpyDeviceToHost));
  *n_host = r;
  return AGP_OK;
}

const char* agp_last_error(agp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

}  // extern "C"

#include "agp_blocks_host.h"
#include "agp_select_host.h"

#define DISPATCH(dtype, call_f64, call_f32)        \
  do {                                             \
    DevGuard _dev_guard(ctx->device);              \
    if ((dtype) == AGP_F64) return call_f64;       \
    if ((dtype) == AGP_F32) return call_f32;       \
    return AGP_ERR_INVALID;                        \
  } while (0)

extern "C" {

agp_status agp_kernelmatrix(agp_ctx* ctx, int32_t dtype, const agp_kernel_desc* k, const void* x, int64_t n, int64_t ldx,
                            const int64_t* idx, const void* y, int64_t p, int64_t ldy, int64_t D, void* out,
                            int64_t ldo) {
  if (!ctx || !k || !x || !out || n <= 0 || D <= 0) return AGP_ERR_INVALID;
  if (k->ard && !k->ard_scales_host) return AGP_ERR_INVALID;
  // leading dimensions are in elements and at least the row width (include/agp_hip.h, "Layout"); the symmetric form is n x n
  if (ldx < D || (y ? (p <= 0 || ldy < D || ldo < p) : ldo < n)) {
    ctx->err = "agp_kernelmatrix: ldx >= D, and with y: p > 0, ldy >= D, ldo >= p; without y: ldo >= n";
    return AGP_ERR_INVALID;
  }
  DISPATCH(dtype, bb_kernelmatrix<double>(ctx, k, x, n, ldx, idx, y, p, ldy, D, out, ldo),
           bb_kernelmatrix<float>(ctx, k, x, n, ldx, idx, y, p, ldy, D, out, ldo));
}

agp_status agp_potrf_jitter(agp_ctx* ctx, int32_t dtype, void* a, int64_t lda, int64_t n, double jitter,
                            int32_t* info_host) {
  if (!ctx || !a || n <= 0 || lda < n) return AGP_ERR_INVALID;
  DISPATCH(dtype, bb_potrf<double>(ctx, a, lda, n, jitter, info_host), bb_potrf<float>(ctx, a, lda, n, jitter, info_host));
}

agp_status agp_spd_inverse(agp_ctx* ctx, int32_t dtype, const void* a, int64_t lda, int64_t n, void* ainv, int64_t ldi,
                           double* logdet_host, int32_t* info_host) {
  if (!ctx || !a || !ainv || n <= 0 || lda < n || ldi < n) return AGP_ERR_INVALID;
  DISPATCH(dtype, bb_spd_inverse<double>(ctx, a, lda, n, ainv, ldi, logdet_host, info_host, nullptr, nullptr),
           bb_spd_inverse<float>(ctx, a, lda, n, ainv, ldi, logdet_host, info_host, nullptr, nullptr));
}

agp_status agp_solve_right_spd(agp_ctx* ctx, int32_t dtype, const void* a, int64_t lda, int64_t n, const void* b,
                               int64_t ldb, int64_t r, void* x, int64_t ldx, int32_t* info_host) {
  if (!ctx || !a || !b || !x || n <= 0 || r <= 0) return AGP_ERR_INVALID;
  if (lda < n || ldb < n || ldx < n) {
    ctx->err = "agp_solve_right_spd: lda, ldb and ldx must be at least n";
    return AGP_ERR_INVALID;
  }
  DISPATCH(dtype, bb_solve_right<double>(ctx, a, lda, n, b, ldb, r, x, ldx, info_host),
           bb_solve_right<float>(ctx, a, lda, n, b, ldb, r, x, ldx, info_host));
}

agp_status agp_mfma_peak(agp_ctx* ctx, int32_t dtype, double* tflops_host) {
  if (!ctx || !tflops_host) return AGP_ERR_INVALID;
  DISPATCH(dtype, bb_mfma_peak<double>(ctx, tflops_host), bb_mfma_peak<float>(ctx, tflops_host));
}

// development micro-benchmark (not part of include/agp_hip.h): microseconds per 64x64 diagonal-tile factorisation
agp_status agp_nearest_center(agp_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t ldx, int64_t D,
                              const void* centers, int64_t ldc, int64_t m, int32_t* labels_out, void* mind_out) {
  if (!ctx) return AGP_ERR_INVALID;
  DISPATCH(dtype, bb_nearest<double>(ctx, x, n, ldx, D, centers, ldc, m, labels_out, mind_out),
           bb_nearest<float>(ctx, x, n, ldx, D, centers, ldc, m, labels_out, mind_out));
}

agp_status agp_kmeans(agp_ctx* ctx, int32_t dtype, const void* x, int64_t n, int64_t ldx, int64_t D, void* centers,
                      int64_t ldc, int64_t m, int32_t max_iter, double tol, int32_t* labels_out, int32_t* counts_out,
                      int32_t* iters_host, double* objective_host, int32_t* converged_host) {
  if (!ctx) return AGP_ERR_INVALID;
  DISPATCH(dtype,
           bb_kmeans<double>(ctx, x, n, ldx, D, centers, ldc, m, max_iter, tol, labels_out, counts_out, iters_host,
                             objective_host, converged_host),
           bb_kmeans<float>(ctx, x, n, ldx, D, centers, ldc, m, max_iter, tol, labels_out, counts_out, iters_host,
                            objective_host, converged_host));
}

agp_status agp_greedy_variance(agp_ctx* ctx, int32_t dtype, const agp_kernel_desc* k, const void* x, int64_t n, int64_t ldx,
                               int64_t D, int64_t m, double tol, int64_t* idx_out, void* z_out, int64_t ldz, void* factor_out,
                               int64_t ldf, double* trace_out, int64_t* n_selected_host) {
  if (!ctx) return AGP_ERR_INVALID;
  // everything is refused before any buffer of the caller is read or written
  const char* bad = nullptr;
  if (!k || !x || !idx_out || !z_out) bad = "null kernel descriptor, x, idx_out or z_out";
  else if (dtype != AGP_F64 && dtype != AGP_F32) bad = "dtype is AGP_F64 or AGP_F32";
  else if (n <= 0 || m <= 0 || m > n) bad = "0 < m <= n";
  else if (D <= 0 || D > GV_MAXD) bad = "0 < D <= 128";
  else if (ldx < D || ldz < D || (factor_out && ldf < m)) bad = "ldx >= D, ldz >= D, ldf >= m";
  else if (!(tol >= 0.0)) bad = "tol >= 0";
  else if (k->kind < AGP_K_SQEXP || k->kind > AGP_K_EXPONENTIAL || !(k->variance > 0.0) || !std::isfinite(k->variance))
    bad = "kernel kind 0..3 and a positive finite variance";
  else if (k->ard && !k->ard_scales_host) bad = "ard without ard_scales_host";
  else {
    for (int64_t d = 0; d < (k->ard ? D : 1); ++d) {
      const double sc = k->ard ? k->ard_scales_host[d] : k->scale;
      if (!(sc > 0.0) || !std::isfinite(sc)) bad = "positive finite kernel scales";
    }
  }
  if (bad) {
    ctx->err = std::string("agp_greedy_variance: ") + bad;
    return AGP_ERR_INVALID;
  }
  DISPATCH(dtype, bb_greedy<double>(ctx, k, x, n, ldx, D, m, tol, idx_out, z_out, ldz, factor_out, ldf, trace_out, n_selected_host),
           bb_greedy<float>(ctx, k, x, n, ldx, D, m, tol, idx_out, z_out, ldz, factor_out, ldf, trace_out, n_selected_host));
}

// development / test hook (not part of include/agp_hip.h): how many task-graph factorisations the in-stream fallback re-ran
agp_status agp_dev_dag_retries(agp_ctx* ctx, int64_t* n) {
  if (!ctx || !n) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  *n = 0;
  if (ctx->safe_retries) {
    int32_t r = 0;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(&r, ctx->safe_retries, sizeof(r), hipMemcpyDeviceToHost));
    *n = r;
  }
  return AGP_OK;
}

agp_status agp_dev_diag_bench(agp_ctx* ctx, int32_t dtype, int32_t variant, int32_t blocks, int32_t reps, double* us) {
  if (!ctx || !us) return AGP_ERR_INVALID;
  const bool f64 = dtype == AGP_F64;
  if (variant != 1 && !(variant == 13 && f64)) return AGP_ERR_INVALID;  // nothing allocated, nothing launched
  DevGuard guard(ctx->device);
  if (!f64) return bb_diag_bench<float, 1>(ctx, blocks, reps, us);
  return variant == 1 ? bb_diag_bench<double, 1>(ctx, blocks, reps, us)    // 2-level, full inverse: k_chol_step, k_chol_safe
                      : bb_diag_bench<double, 13>(ctx, blocks, reps, us);  // 2-level without X21: the chain of k_chol_dag
}

agp_status agp_svgp_create(agp_ctx* ctx, const agp_svgp_desc* desc, agp_svgp** out) {
  if (!ctx || !desc || !out) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  *out = nullptr;
  SvgpBase* impl = nullptr;
  if ((desc->flags & AGP_FLAG_FULL) && desc->dtype != AGP_F64) {
    ctx->err = "AGP_FLAG_FULL: the full model is Float64 only";
    return AGP_ERR_UNSUPPORTED;
  }
  if ((desc->flags & AGP_FLAG_EXACT) && !(desc->flags & AGP_FLAG_FULL)) {
    ctx->err = "AGP_FLAG_EXACT: exact GP regression is a full model (AGP_FLAG_FULL | AGP_FLAG_EXACT)";
    return AGP_ERR_UNSUPPORTED;
  }
  if ((desc->flags & AGP_FLAG_SAMPLED) && (!(desc->flags & AGP_FLAG_FULL) || (desc->flags & AGP_FLAG_EXACT))) {
    ctx->err = std::string("AGP_FLAG_SAMPLED: Gibbs sampling runs on the full model (AGP_FLAG_FULL | AGP_FLAG_SAMPLED, without "
                           "AGP_FLAG_EXACT); ") + Mcgp::supported();
    return AGP_ERR_UNSUPPORTED;
  }
  if ((desc->flags & AGP_FLAG_NUMERICAL) && ((desc->flags & (AGP_FLAG_EXACT | AGP_FLAG_SAMPLED)) || desc->dtype != AGP_F64)) {
    ctx->err = std::string("AGP_FLAG_NUMERICAL: ") + ((desc->flags & AGP_FLAG_MC) ? mc_supported() : nvi_supported()) +
               " (never with AGP_FLAG_EXACT or AGP_FLAG_SAMPLED)";
    return AGP_ERR_UNSUPPORTED;
  }
  if ((desc->flags & AGP_FLAG_MC) && !(desc->flags & AGP_FLAG_NUMERICAL)) {
    ctx->err = std::string("AGP_FLAG_MC is valid only together with AGP_FLAG_NUMERICAL (with or without AGP_FLAG_FULL); ") + mc_supported();
    return AGP_ERR_UNSUPPORTED;
  }
  if (desc->flags & AGP_FLAG_NUMERICAL) impl = (desc->flags & AGP_FLAG_FULL) ? new Nvgp() : new Nsvgp();
  else if (desc->flags & AGP_FLAG_SAMPLED) impl = new Mcgp();
  else if (desc->flags & AGP_FLAG_EXACT) impl = new Gp();
  else if (desc->flags & AGP_FLAG_FULL) impl = desc->lik.kind == AGP_LIK_MULTIOUTPUT ? new Movgp() : new Vgp();
  else if (desc->dtype == AGP_F64) impl = new Svgp<double>();
  else if (desc->dtype == AGP_F32) impl = new Svgp<float>();
  else return AGP_ERR_INVALID;
  impl->ctx = ctx;
  impl->desc = *desc;
  agp_status s = impl->init();
  if (s != AGP_OK) {
    delete impl;
    return s;
  }
  agp_svgp* h = new agp_svgp();
  h->impl = impl;
  *out = h;
  return AGP_OK;
}

agp_status agp_svgp_destroy(agp_svgp* h) {
  if (!h) return AGP_OK;
  DevGuard guard(h->impl->ctx->device);
  (void)hipStreamSynchronize(h->impl->ctx->stream);
  delete h->impl;
  delete h;
  return AGP_OK;
}

#define HCHK(h)                                    \
  if (!(h) || !(h)->impl) return AGP_ERR_INVALID;  \
  DevGuard _dev_guard((h)->impl->ctx->device)
// ... and, for every entry point outside the CAVI step / look-ahead pair: take a pending natural-gradient step first
#define HCHKF(h) \
  HCHK(h);       \
  AGPCHK((h)->impl->flush())
// entry points that have no meaning for a full model (AGP_FLAG_FULL): refused, nothing done
static agp_status full_refused(agp_svgp* h, const char* what) {
  h->impl->ctx->err = std::string((h)->impl->desc.flags & AGP_FLAG_FULL ? "full model (AGP_FLAG_FULL): "
                                                                          : "numerical inference (AGP_FLAG_NUMERICAL): ") +
                      what + " is not supported";
  return AGP_ERR_UNSUPPORTED;
}
// (... nor for a handle that runs numerical inference, full or sparse: it has no CAVI phases, look-ahead, shards or kappa buffers)
#define FULLNO(h, what) \
  if ((h)->impl->desc.flags & (AGP_FLAG_FULL | AGP_FLAG_NUMERICAL)) return full_refused((h), (what))
// ... the mixing weights' entry points: refused unless the full model is the multi-output one (Movgp)
#define FULLNO_SINGLE(h, what)                                                                                  \
  if (((h)->impl->desc.flags & AGP_FLAG_FULL) && (h)->impl->desc.lik.kind != AGP_LIK_MULTIOUTPUT) \
  return full_refused((h), (what))
// ... and those that have none for exact GP regression (AGP_FLAG_EXACT) on top of them
static agp_status exact_refused(agp_svgp* h, const char* what) {
  h->impl->ctx->err = std::string("exact GP (AGP_FLAG_EXACT): ") + what + " is not supported";
  return AGP_ERR_UNSUPPORTED;
}
#define EXACTNO(h, what) \
  if ((h)->impl->desc.flags & AGP_FLAG_EXACT) return exact_refused((h), (what))

agp_status agp_svgp_set_kernel(agp_svgp* h, int32_t latent, const agp_kernel_desc* k) {
  HCHKF(h);
  return h->impl->set_kernel(latent, k);
}
agp_status agp_svgp_set_Z(agp_svgp* h, int32_t latent, const void* z, int64_t ldz) {
  HCHKF(h);
  return h->impl->set_Z(latent, z, ldz);
}
agp_status agp_svgp_get_Z(agp_svgp* h, int32_t latent, void* z, int64_t ldz) {
  HCHKF(h);
  return h->impl->get_Z(latent, z, ldz);
}
agp_status agp_svgp_set_prior_mean(agp_svgp* h, int32_t latent, const void* mu0) {
  HCHKF(h);
  return h->impl->set_mu0(latent, mu0);
}
agp_status agp_svgp_refresh_K(agp_svgp* h) {
  HCHKF(h);
  return h->impl->refresh_K_explicit();
}
agp_status agp_svgp_set_opt_state(agp_svgp* h, int64_t n) {
  HCHK(h);
  if (n < 1) return AGP_ERR_INVALID;
  h->impl->n_opt = n;
  return AGP_OK;
}
agp_status agp_svgp_get_opt_state(agp_svgp* h, int64_t* n_host) {
  HCHK(h);
  *n_host = h->impl->n_opt;
  return AGP_OK;
}

agp_status agp_svgp_cavi_step(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                              double rho) {
  HCHK(h);
  SvgpBase* s = h->impl;
  s->in_cavi_step = true;
  const agp_status sl_ = s->step_local(x, ldx, y, idx, B, rho, false);
  s->in_cavi_step = false;
  AGPCHK(sl_);
  AGPCHK(s->lsm_local_all());
  s->n_steps += 1;
  return s->step_finish();
}
agp_status agp_svgp_step_counters(agp_svgp* h, int64_t* n_steps_host, int64_t* n_prologue_host) {
  HCHK(h);
  if (n_steps_host) *n_steps_host = h->impl->n_steps;
  if (n_prologue_host) *n_prologue_host = h->impl->n_prologue;
  return AGP_OK;
}

agp_status agp_svgp_hyper_counters(agp_svgp* h, int64_t* n_grad_host, int64_t* n_gk_fused_host) {
  HCHK(h);
  if (n_grad_host) *n_grad_host = h->impl->n_hgrad;
  if (n_gk_fused_host) *n_gk_fused_host = h->impl->n_gk_fused;
  return AGP_OK;
}

agp_status agp_svgp_step_local(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                               double rho) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_step_local");
  return h->impl->step_local(x, ldx, y, idx, B, rho, false);
}
agp_status agp_svgp_prefetch(agp_svgp* h, const void* x, int64_t ldx, const int64_t* idx, int64_t B) {
  HCHK(h);
  FULLNO(h, "agp_svgp_prefetch");
  return h->impl->prefetch(x, ldx, idx, B);
}
agp_status agp_svgp_set_multioutput(agp_svgp* h, int32_t n_task, const agp_lik_desc* liks_host, const double* A_host,
                                    double adam_eta, double adam_b1, double adam_b2, double adam_eps) {
  HCHKF(h);
  FULLNO_SINGLE(h, "agp_svgp_set_multioutput");
  return h->impl->set_multioutput(n_task, liks_host, A_host, adam_eta, adam_b1, adam_b2, adam_eps);
}
agp_status agp_svgp_get_A(agp_svgp* h, double* A_host) {
  HCHKF(h);
  FULLNO_SINGLE(h, "agp_svgp_get_A");
  return h->impl->get_A(A_host);
}
agp_status agp_svgp_elbo_terms(agp_svgp* h, double* terms_host) {
  HCHKF(h);
  EXACTNO(h, "agp_svgp_elbo_terms");
  return h->impl->elbo_terms(terms_host);
}
agp_status agp_svgp_set_batch_shard(agp_svgp* h, int32_t rank, int32_t world) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_set_batch_shard");
  return h->impl->set_batch_shard(rank, world);
}
agp_status agp_svgp_mo_shard(agp_svgp* h, int32_t q_total) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_mo_shard");
  return h->impl->mo_shard(q_total);
}
agp_status agp_svgp_mo_fbuf_ptr(agp_svgp* h, void** ptr, int64_t* count) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_mo_fbuf_ptr");
  return h->impl->mo_fbuf_ptr(ptr, count);
}
agp_status agp_svgp_mo_mix(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_mo_mix");
  return h->impl->mo_mix();
}
agp_status agp_svgp_mo_refresh_f(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_mo_refresh_f");
  return h->impl->mo_refresh_f();
}
agp_status agp_svgp_mo_predict_from_f(agp_svgp* h, int64_t n_t, int32_t mode, void* out0, void* out1,
                                      const double* gh_nodes_host, const double* gh_weights_host, int32_t n_nodes) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_mo_predict_from_f");
  return h->impl->mo_predict_from_f(n_t, mode, out0, out1, gh_nodes_host, gh_weights_host, n_nodes);
}
agp_status agp_svgp_elbo_enqueue(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho,
                                 int32_t fresh_local, int32_t* ticket) {
  HCHKF(h);
  EXACTNO(h, "agp_svgp_elbo_enqueue");
  return h->impl->elbo_enqueue(x, ldx, y, idx, B, rho, fresh_local, ticket);
}
agp_status agp_svgp_elbo_fetch(agp_svgp* h, int32_t ticket, int32_t wait, double* out_host, int32_t* ready) {
  HCHK(h);
  return h->impl->elbo_fetch(ticket, wait, out_host, ready);
}

agp_status agp_svgp_hyper_rule(agp_svgp* h, int32_t kernel_rule, double kernel_rho, int32_t z_rule, double z_rho) {
  HCHK(h);
  return h->impl->hyper_rule(kernel_rule, kernel_rho, z_rule, z_rho);
}

agp_status agp_svgp_hyper_configure(agp_svgp* h, int32_t opt_kernel, double kernel_eta, int32_t opt_Z, double z_eta,
                                    double adam_b1, double adam_b2, double adam_eps) {
  HCHKF(h);
  if (opt_Z) FULLNO(h, "optimising the training inputs (opt_Z)");
  return h->impl->hyper_configure(opt_kernel, kernel_eta, opt_Z, z_eta, adam_b1, adam_b2, adam_eps);
}
agp_status agp_svgp_hypergrad(agp_svgp* h, int32_t latent, double* dvariance_host, double* dscale_host, void* dZ) {
  HCHKF(h);
  return h->impl->hypergrad(latent, dvariance_host, dscale_host, dZ);
}
agp_status agp_svgp_hyper_step(agp_svgp* h) {
  HCHK(h);  // (no flush: a pending natural-gradient step becomes the prologue of the factorisation the gradient needs, aug_factor)
  return h->impl->hyper_step();
}
agp_status agp_svgp_get_kernel(agp_svgp* h, int32_t latent, double* variance_host, double* scales_host) {
  HCHKF(h);
  return h->impl->get_kernel(latent, variance_host, scales_host);
}
agp_status agp_svgp_lsm_gamma(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_lsm_gamma");
  return h->impl->lsm_gamma();
}
agp_status agp_svgp_lsm_alpha(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_lsm_alpha");
  return h->impl->lsm_alpha();
}
agp_status agp_svgp_lsm_gsum_ptr(agp_svgp* h, void** ptr, int64_t* count) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_lsm_gsum_ptr");
  return h->impl->lsm_gsum_ptr(ptr, count);
}
agp_status agp_svgp_step_stats(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_step_stats");
  return h->impl->step_stats(false);
}
#ifdef AGP_DEBUG_PTRS
void* agp_debug_ptr(agp_svgp* h, int what) { return (h && h->impl) ? h->impl->debug_ptr(what) : nullptr; }
// the words of agp_dag_diag (agp_chol.h) + [6] the context's flag block, [7] int32 words per flag, DAG_FS (so that [1] can be turned
// into a flag index: ([1] - [6]) / 4 / [7]); synchronises the device
int agp_debug_dag_diag(agp_ctx* c, unsigned long long* out8) {
  if (!out8) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return 2;
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(agp_dag_diag), 8 * sizeof(unsigned long long)) != hipSuccess) return 3;
  out8[6] = c ? (unsigned long long)c->dag_flags : 0ull;
  out8[7] = (unsigned long long)DAG_FS;
  return 0;
}
#endif
agp_status agp_svgp_stats_ptr(agp_svgp* h, void** ptr, int64_t* count) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_stats_ptr");
  return h->impl->stats_ptr(ptr, count);
}
agp_status agp_svgp_step_global(agp_svgp* h) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_step_global");
  return h->impl->step_global(false);
}
agp_status agp_svgp_timing_enable(agp_svgp* h, int32_t on) {
  HCHK(h);
  h->impl->timing = on != 0;
  h->impl->timing_every = on > 1 ? on : 1;
  h->impl->timing_ctr = 0;
  return AGP_OK;
}
agp_status agp_svgp_timing_read(agp_svgp* h, int64_t* n_launches_host, double* total_ms_host) {
  HCHK(h);
  if (!n_launches_host || !total_ms_host) return AGP_ERR_INVALID;
  return h->impl->timing_read(n_launches_host, total_ms_host);
}
agp_status agp_svgp_check_status(agp_svgp* h) {
  HCHKF(h);
  return h->impl->check_status();
}
agp_status agp_svgp_elbo(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B,
                         double rho, int32_t fresh_local, double* elbo_host) {
  HCHKF(h);
  if (!elbo_host) return AGP_ERR_INVALID;
  return h->impl->elbo(x, ldx, y, idx, B, rho, fresh_local, elbo_host);
}
agp_status agp_svgp_elbo_stream(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t n,
                                double rho, double* elbo_host, double* terms_host) {
  HCHKF(h);
  return h->impl->elbo_stream(x, ldx, y, idx, n, rho, elbo_host, terms_host);
}
agp_status agp_svgp_lpd_stream(agp_svgp* h, const void* xt, int64_t ldx, const void* y, int64_t n, const double* gh_nodes_host,
                               const double* gh_weights_host, int32_t n_nodes, double* sum_host, void* lpd_out) {
  HCHKF(h);
  return h->impl->lpd_stream(xt, ldx, y, n, gh_nodes_host, gh_weights_host, n_nodes, sum_host, lpd_out);
}
agp_status agp_log_predictive(agp_ctx* ctx, int32_t dtype, const agp_lik_desc* lik, const void* y, const void* mu, const void* var,
                              int64_t n, int64_t ld, const double* gh_nodes_host, const double* gh_weights_host, int32_t n_nodes,
                              void* lpd_out) {
  if (!ctx) return AGP_ERR_INVALID;
  const char* who = "agp_log_predictive";
  if (!lik || (dtype != AGP_F64 && dtype != AGP_F32) || n < 0 || (n > 0 && (!y || !mu || !var || !lpd_out || ld < n))) {
    ctx->err = "agp_log_predictive: lik, y, mu, var and lpd_out must not be NULL, dtype AGP_F64 / AGP_F32, n >= 0, ld >= n";
    return AGP_ERR_INVALID;
  }
  if (!lpd_lik_ok(lik->kind)) {
    ctx->err = "agp_log_predictive: Gaussian, Laplace, Logistic, BayesianSVM, StudentT, Poisson, NegBinomial, LogisticSoftMax and "
               "SoftMax are supported (Heteroscedastic: a follow-up)";
    return AGP_ERR_UNSUPPORTED;
  }
  if (lpd_is_multiclass(lik->kind) && lik->n_class < 1) {
    ctx->err = "agp_log_predictive: n_class must be positive";
    return AGP_ERR_INVALID;
  }
  LpdParams P;
  AGPCHK(lpd_params(ctx, who, *lik, &P));
  if (n == 0) return AGP_OK;
  DevGuard guard(ctx->device);
  LpdRule rule;
  if (lpd_is_quad(lik->kind)) AGPCHK(rule.ensure(ctx, who, ctx->stream, gh_nodes_host, gh_weights_host, n_nodes));
  const int nl = lpd_is_multiclass(lik->kind) ? lik->n_class : 1;
  const int64_t ppb = lpd_points_per_block(lik->kind), nw = (n + ppb - 1) / ppb;
  double* ws = nullptr;  // partials | out[3] of the reduction, padding | the two failure words
  AGPCHK(dmalloc(ctx, &ws, nw + 8));
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(ws + nw + 4);
  double h[3] = {0.0, -1.0, -1.0};
  agp_status st = AGP_OK;
  hipError_t e = hipMemsetAsync(bad, 0xFF, 2 * sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) {
    st = dtype == AGP_F32 ? lpd_launch<float>(ctx, ctx->stream, lik->kind, n, 0, nl, ld, P, nullptr, y, (const float*)mu,
                                              (const float*)var, rule.dev, n_nodes, (float*)lpd_out, ws, bad)
                          : lpd_launch<double>(ctx, ctx->stream, lik->kind, n, 0, nl, ld, P, nullptr, y, (const double*)mu,
                                               (const double*)var, rule.dev, n_nodes, (double*)lpd_out, ws, bad);
    if (st == AGP_OK) {
      hipLaunchKernelGGL(k_lpd_reduce, dim3(1), dim3(1024), 0, ctx->stream, (const double*)ws, nw, (const unsigned long long*)bad,
                         ws + nw);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && st == AGP_OK) e = hipMemcpyAsync(h, ws + nw, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream);
  // (ws and the rule's buffers are released below: the stream is drained first, on every path)
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  (void)hipFree(ws);
  if (st != AGP_OK) return st;
  if (e != hipSuccess || e2 != hipSuccess) {
    ctx->err = std::string("agp_log_predictive: ") + hipGetErrorString(e != hipSuccess ? e : e2);
    return AGP_ERR_HIP;
  }
  return lpd_failure(ctx, who, h);
}
agp_status agp_svgp_get_state(agp_svgp* h, int32_t latent, void* mu, void* sigma, void* eta1, void* eta2) {
  HCHKF(h);
  return h->impl->get_state(latent, mu, sigma, eta1, eta2);
}
agp_status agp_svgp_set_state(agp_svgp* h, int32_t latent, const void* eta1, const void* eta2) {
  HCHKF(h);
  return h->impl->set_state(latent, eta1, eta2);
}
agp_status agp_svgp_get_matrix(agp_svgp* h, int32_t latent, int32_t which, void* out, int64_t ldo, int64_t cap) {
  HCHKF(h);
  if (which == AGP_VEC_APRED || which == AGP_MAT_APRED) return h->impl->get_predictor(latent, which, out, ldo, cap);  // every class
  if (h->impl->desc.flags & AGP_FLAG_EXACT) return exact_refused(h, "agp_svgp_get_matrix");
  if (which == AGP_MAT_KNM || which == AGP_MAT_KAPPA) FULLNO(h, "K_nm / kappa (kappa = I)");
  return h->impl->get_matrix(latent, which, out, ldo, cap);
}
agp_status agp_svgp_last_batch(agp_svgp* h, int64_t* B_host) {
  HCHK(h);
  if (!B_host) return AGP_ERR_INVALID;
  *B_host = h->impl->last_batch();
  return AGP_OK;
}
agp_status agp_svgp_invalidate_data(agp_svgp* h) {
  HCHKF(h);
  return h->impl->invalidate_data();
}
agp_status agp_svgp_init_state(agp_svgp* h) {
  HCHKF(h);
  return h->impl->init_state();
}
agp_status agp_svgp_predict_f_cov(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* mu_out, void* cov_out) {
  HCHKF(h);
  if (n_t == 0) return AGP_OK;  // no test points: nothing to write (the reference returns empty arrays)
  return h->impl->predict_f_cov(xt, ldx, n_t, mu_out, cov_out);
}
agp_status agp_svgp_predict_f(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* mu_out, void* var_out) {
  HCHKF(h);
  if (n_t == 0) return AGP_OK;  // no test points: nothing to write (the reference returns empty arrays)
  return h->impl->predict_f(xt, ldx, n_t, mu_out, var_out);
}
agp_status agp_svgp_predict_f_grad(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* dmu_out, void* dvar_out,
                                   int64_t ldg) {
  HCHKF(h);
  return h->impl->predict_f_grad(xt, ldx, n_t, dmu_out, dvar_out, ldg);
}
// ---- acquisition functions ("ACQUISITION FUNCTIONS") ----------------------------------------------------------------------------
agp_status agp_acq_moments(agp_ctx* ctx, const agp_acq_desc* desc, int64_t n, const void* mu, const void* var, void* alpha_out,
                           void* dalpha_dmu, void* dalpha_dvar) {
  if (!ctx) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  return acq_moments(ctx, desc, n, (const double*)mu, (const double*)var, (double*)alpha_out, (double*)dalpha_dmu, (double*)dalpha_dvar);
}
agp_status agp_svgp_acquisition(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xt, int64_t ldx, int64_t n_t,
                                void* alpha_out, void* grad_out, int64_t ldg) {
  HCHKF(h);
  return AcqDriver::evaluate(*h->impl, latent, desc, (const double*)xt, ldx, n_t, (double*)alpha_out, (double*)grad_out, ldg);
}
agp_status agp_svgp_acq_maximize(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* x0, int64_t ldx0, int64_t n_starts,
                                 const agp_pw_ascent_opts* opts, void* x_out, int64_t ldxo, void* a_out, void* best_x, void* best_a,
                                 void* best_idx) {
  HCHKF(h);
  return AcqDriver::maximize(*h->impl, latent, desc, (const double*)x0, ldx0, n_starts, opts, (double*)x_out, ldxo, (double*)a_out,
                             (double*)best_x, (double*)best_a, (int64_t*)best_idx);
}
agp_status agp_svgp_acquisition_pending(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xp, int64_t ldp,
                                        int64_t n_pending, double noise, const void* xt, int64_t ldx, int64_t n_t, void* alpha_out,
                                        void* grad_out, int64_t ldg) {
  HCHKF(h);
  return AcqDriver::evaluate_pending(*h->impl, latent, desc, (const double*)xp, ldp, n_pending, noise, (const double*)xt, ldx, n_t,
                                     (double*)alpha_out, (double*)grad_out, ldg);
}
agp_status agp_svgp_acq_maximize_batch(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xp, int64_t ldp,
                                       int64_t n_pending, double noise, int64_t q, const void* x0, int64_t ldx0, int64_t n_starts,
                                       const agp_pw_ascent_opts* opts, void* xb_out, int64_t ldxb, void* ab_out, void* idxb_out) {
  HCHKF(h);
  return AcqDriver::maximize_batch(*h->impl, latent, desc, (const double*)xp, ldp, n_pending, noise, q, (const double*)x0, ldx0,
                                   n_starts, opts, (double*)xb_out, ldxb, (double*)ab_out, (int64_t*)idxb_out);
}
agp_status agp_svgp_predict_y(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, void* y_out) {
  HCHKF(h);
  if (n_t == 0) return AGP_OK;  // no test points: nothing to write (the reference returns empty arrays)
  return h->impl->predict_y(xt, ldx, n_t, y_out);
}

// ---- Gibbs sampling (AGP_FLAG_FULL | AGP_FLAG_SAMPLED) -----------------------------------------------------------------------
agp_status agp_svgp_gibbs_sample(agp_svgp* h, const void* y, int64_t n_samples, int64_t discard_initial, int64_t thinning,
                                 uint64_t seed, void* store, int64_t lds) {
  HCHK(h);
  return h->impl->gibbs_sample(y, n_samples, discard_initial, thinning, seed, store, lds);
}
agp_status agp_svgp_gibbs_counter(agp_svgp* h, int32_t set, int64_t* t_host) {
  HCHK(h);
  return h->impl->gibbs_counter(set, t_host);
}
agp_status agp_svgp_predict_samples(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, const void* store, int64_t lds,
                                    int64_t n_samples, int32_t mode, void* out0, void* out1) {
  HCHK(h);
  if (n_t == 0) return AGP_OK;
  return h->impl->predict_samples(xt, ldx, n_t, store, lds, n_samples, mode, out0, out1);
}
agp_status agp_sample_local(agp_ctx* ctx, const agp_lik_desc* lik, const void* y, const void* f, int64_t n, uint64_t seed,
                            int64_t t, void* theta_out, void* aux_out) {
  if (!ctx || !lik || !y || !f || !theta_out || n < 0 || n > (int64_t)0xFFFFFFFFll || t < 0 || t > (int64_t)0xFFFFFFFFll)
    return AGP_ERR_INVALID;
  if (lik->kind != AGP_LIK_LOGISTIC && lik->kind != AGP_LIK_STUDENTT && lik->kind != AGP_LIK_NEGBINOMIAL) {
    ctx->err = std::string("agp_sample_local: ") + Mcgp::supported();
    return AGP_ERR_UNSUPPORTED;
  }
  if ((lik->kind == AGP_LIK_STUDENTT && !(lik->p0 > 0.5)) ||
      (lik->kind == AGP_LIK_NEGBINOMIAL && !(lik->p0 > 0 && lik->p0 == std::floor(lik->p0)))) {
    ctx->err = "agp_sample_local: StudentT needs nu > 0.5, NegBinomial a positive integer r";
    return AGP_ERR_INVALID;
  }
  if (n == 0) return AGP_OK;
  DevGuard guard(ctx->device);
  int* flag = nullptr;
  AGPCHK(dmalloc(ctx, &flag, 1));
  LikParams<double> lp{};
  lp.kind = lik->kind;
  lp.p0 = lik->p0;
  lp.p1 = lik->p1;
  int host = 0;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL((k_gibbs_local<double>), grid1(n), dim3(256), 0, ctx->stream, n, lp, (const double*)y, (const double*)f, seed,
                       (uint32_t)t, (double*)theta_out, (double*)aux_out, (double*)nullptr, (double*)nullptr, flag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(flag);
  if (e != hipSuccess) {
    ctx->err = std::string("agp_sample_local: ") + hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  if (host & FLAG_BAD_COUNT) {
    ctx->err = "agp_sample_local: the targets of a NegBinomial likelihood must be non-negative integers (PolyaGamma(y + r, |f|))";
    return AGP_ERR_LABELS;
  }
  if (host & FLAG_RNG_BOUND) {
    ctx->err = "agp_sample_local: a variate sampler ran into its iteration bound (agp_rand.h)";
    return AGP_ERR_HIP;
  }
  return AGP_OK;
}

// ---- numerical inference (AGP_FLAG_FULL | AGP_FLAG_NUMERICAL) ------------------------------------------------------------------
agp_status agp_svgp_nvi_configure(agp_svgp* h, int32_t n, const double* nodes_host, const double* weights_host, int32_t natural,
                                  int32_t opt_kind, double eta, double p1, double p2, double eps) {
  HCHK(h);
  return h->impl->nvi_configure(n, nodes_host, weights_host, natural, opt_kind, eta, p1, p2, eps);
}
agp_status agp_svgp_nvi_step(agp_svgp* h, const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho) {
  HCHK(h);
  return h->impl->nvi_step(x, ldx, y, idx, B, rho);
}
agp_status agp_svgp_nvi_info(agp_svgp* h, int32_t latent, double* alpha_last_host, int64_t* halvings_total_host,
                             int64_t* rejected_total_host) {
  HCHK(h);
  return h->impl->nvi_info(latent, alpha_last_host, halvings_total_host, rejected_total_host);
}
agp_status agp_svgp_nvi_state(agp_svgp* h, int32_t latent, int32_t set, void* mom_mu, void* mom_sigma, int64_t* t_host) {
  HCHK(h);
  return h->impl->nvi_state(latent, set, mom_mu, mom_sigma, t_host);
}
agp_status agp_quad_expectations(agp_ctx* ctx, const agp_lik_desc* lik, const void* y, const void* mu, const void* var, int64_t n_pts,
                                 const double* nodes_host, const double* weights_host, int32_t n, void* ell, void* g, void* h) {
  if (!ctx || !lik || !y || !mu || !var || !nodes_host || !weights_host || !ell || !g || !h || n_pts < 0 || n < 1 || n > 4096)
    return AGP_ERR_INVALID;
  if (!nvi_lik_ok(lik->kind)) {
    ctx->err = std::string("agp_quad_expectations: ") + nvi_supported();
    return AGP_ERR_UNSUPPORTED;
  }
  if ((lik->kind == AGP_LIK_STUDENTT && !(lik->p0 > 0.5 && lik->p1 > 0)) || (lik->kind == AGP_LIK_LAPLACE && !(lik->p0 > 0))) {
    ctx->err = "agp_quad_expectations: StudentT needs nu > 0.5 and sigma > 0, Laplace beta > 0";
    return AGP_ERR_INVALID;
  }
  if (n_pts == 0) return AGP_OK;
  DevGuard guard(ctx->device);
  double* q = nullptr;
  AGPCHK(dmalloc(ctx, &q, 2 * (int64_t)n));
  LikParams<double> lp{};
  lp.kind = lik->kind;
  lp.p0 = lik->p0;
  lp.p1 = lik->p1;
  hipError_t e = hipMemcpyAsync(q, nodes_host, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(q + n, weights_host, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL((k_quad_local<double>), grid1(n_pts), dim3(256), 0, ctx->stream, n_pts, lp, nvi_lconst(lik->kind, lik->p0),
                       (const double*)y, (const int64_t*)nullptr, (const double*)mu, (const double*)var, (const double*)q, (const double*)(q + n), (int)n,
                       (double*)ell, (double*)g, (double*)h);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(q);
  if (e != hipSuccess) {
    ctx->err = std::string("agp_quad_expectations: ") + hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  return AGP_OK;
}

// ---- Monte-Carlo integration (AGP_FLAG_NUMERICAL | AGP_FLAG_MC) ------------------------------------------------------------------
agp_status agp_svgp_mcvi_configure(agp_svgp* h, int32_t nMC, uint64_t seed, int32_t natural, int32_t opt_kind, double eta, double p1,
                                   double p2, double eps) {
  HCHK(h);
  return h->impl->mcvi_configure(nMC, seed, natural, opt_kind, eta, p1, p2, eps);
}
static bool mc_table_args_ok(int64_t t, int32_t stream, int32_t nMC, int32_t K) {
  return t >= 0 && t <= (int64_t)0xFFFFFFFFll && stream >= 0 && nMC >= 1 && nMC <= 65536 && K >= 1 &&
         (int64_t)nMC * K <= (int64_t)0xFFFFFFFFll;
}
agp_status agp_mc_normals(agp_ctx* ctx, uint64_t seed, int64_t t, int32_t stream, int32_t nMC, int32_t K, void* out) {
  if (!ctx || !out || !mc_table_args_ok(t, stream, nMC, K)) return AGP_ERR_INVALID;
  DevGuard guard(ctx->device);
  AGPCHK(mc_fill_normals(ctx, ctx->stream, seed, t, stream, nMC, K, (double*)out));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}
agp_status agp_mc_expectations(agp_ctx* ctx, const agp_lik_desc* lik, const void* y_class, const void* mu, const void* var,
                               int64_t n_pts, int32_t K, int32_t nMC, uint64_t seed, int64_t t, int32_t stream, void* ell, void* g,
                               void* h) {
  if (!ctx || !lik || !y_class || !mu || !var || !ell || !g || !h || n_pts < 0 || !mc_table_args_ok(t, stream, nMC, K))
    return AGP_ERR_INVALID;
  if (!mc_lik_ok(lik->kind) || K < 2 || K > MC_KMAX || lik->n_class != K) {
    ctx->err = std::string("agp_mc_expectations: ") + mc_supported();
    return AGP_ERR_UNSUPPORTED;
  }
  if (n_pts == 0) return AGP_OK;
  DevGuard guard(ctx->device);
  double* tab = nullptr;
  AGPCHK(dmalloc(ctx, &tab, (int64_t)nMC * K + 1));
  int* flag = (int*)(tab + (int64_t)nMC * K);
  int host = 0;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(double), ctx->stream);
  if (e == hipSuccess) {
    const int64_t n = (int64_t)nMC * K;
    hipLaunchKernelGGL(k_mc_normals, grid1(n), dim3(256), 0, ctx->stream, n, seed, (uint32_t)t, (uint32_t)stream, tab);
    hipLaunchKernelGGL(k_mc_local, dim3((unsigned)((n_pts + 3) / 4)), dim3(256), 0, ctx->stream, n_pts, (int)lik->kind, (int)K, (int)nMC,
                       (const int32_t*)y_class, (const int64_t*)nullptr, (const double*)mu, (const double*)var, n_pts, (const double*)tab,
                       (double*)ell, (double*)g, (double*)h, n_pts, flag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(tab);
  if (e != hipSuccess) {
    ctx->err = std::string("agp_mc_expectations: ") + hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  if (host & FLAG_BAD_LABEL) {
    ctx->err = "agp_mc_expectations: a class index outside [0, K)";
    return AGP_ERR_LABELS;
  }
  return AGP_OK;
}

// ---- pathwise sampling ----------------------------------------------------------------------------------------------------------
agp_status agp_svgp_pathwise_draw(agp_svgp* h, int32_t n_features, int32_t n_samples, uint64_t seed, int64_t t, agp_pathwise** out) {
  HCHK(h);
  return h->impl->pathwise_draw(n_features, n_samples, seed, t, out);
}
agp_status agp_pathwise_eval(agp_pathwise* p, const void* xt, int64_t ldx, int64_t n_t, void* out, int64_t ldo) {
  if (!p) return AGP_ERR_INVALID;
  if (n_t == 0) return AGP_OK;
  if (!xt || !out || n_t < 0 || ldx < p->D || ldo < n_t) {
    p->ctx->err = "agp_pathwise_eval: xt and out must be given, n_t >= 0, ldx >= D, ldo >= n_t";
    return AGP_ERR_INVALID;
  }
  DevGuard guard(p->ctx->device);
  return pw_eval(*p, (const double*)xt, ldx, n_t, (double*)out, ldo);
}
agp_status agp_pathwise_eval_grad(agp_pathwise* p, const void* xt, int64_t ldx, int64_t n_t, void* f_out, int64_t ldo, void* g_out,
                                  int64_t lds, int64_t ldg) {
  if (!p) return AGP_ERR_INVALID;
  if (n_t == 0) return AGP_OK;
  const char* bad = nullptr;
  if (!xt) bad = "xt must be given";
  else if (!g_out) bad = "g_out must be given";
  else if (n_t < 0) bad = "n_t >= 0";
  else if (ldx < p->D) bad = "ldx >= D";
  else if (lds < n_t) bad = "lds >= n_t";
  else if (ldg < p->D) bad = "ldg >= D";
  else if (f_out && ldo < n_t) bad = "ldo >= n_t when f_out is given";
  if (bad) {
    p->ctx->err = std::string("agp_pathwise_eval_grad: ") + bad;
    return AGP_ERR_INVALID;
  }
  DevGuard guard(p->ctx->device);
  return pw_eval_grad(*p, (const double*)xt, ldx, n_t, (double*)f_out, ldo, (double*)g_out, lds, ldg);
}
agp_status agp_pathwise_maximize(agp_pathwise* p, int32_t latent, const void* x0, int64_t ldx0, int64_t n_starts,
                                 const agp_pw_ascent_opts* opts, void* x_out, int64_t ldxo, void* f_out, int64_t ldf, void* best_x,
                                 int64_t ldb, void* best_f, void* best_idx) {
  if (!p) return AGP_ERR_INVALID;
  DevGuard guard(p->ctx->device);
  return pw_maximize(p, latent, (const double*)x0, ldx0, n_starts, opts, (double*)x_out, ldxo, (double*)f_out, ldf, (double*)best_x, ldb,
                     (double*)best_f, (int64_t*)best_idx);
}
agp_status agp_svgp_acquisition_joint(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xp, int64_t ldp,
                                      int64_t n_pending, int64_t q, const void* xq, int64_t ldx, int64_t n_sets, const void* eps,
                                      int64_t lde, int64_t S, void* alpha_out, void* grad_out, int64_t ldg) {
  HCHK(h);
  return AcqJointDriver::evaluate(*h->impl, latent, desc, (const double*)xp, ldp, n_pending, q, (const double*)xq, ldx, n_sets,
                                  (const double*)eps, lde, S, (double*)alpha_out, (double*)grad_out, ldg);
}
agp_status agp_svgp_acq_maximize_joint(agp_svgp* h, int32_t latent, const agp_acq_desc* desc, const void* xp, int64_t ldp,
                                       int64_t n_pending, int64_t q, const void* x0, int64_t ldx0, int64_t n_starts, const void* eps,
                                       int64_t lde, int64_t S, const agp_pw_ascent_opts* opts, void* x_out, int64_t ldxo, void* a_out,
                                       void* best_x, int64_t ldb, void* best_a, void* best_idx) {
  HCHK(h);
  return AcqJointDriver::maximize(*h->impl, latent, desc, (const double*)xp, ldp, n_pending, q, (const double*)x0, ldx0, n_starts,
                                  (const double*)eps, lde, S, opts, (double*)x_out, ldxo, (double*)a_out, (double*)best_x, ldb,
                                  (double*)best_a, (int64_t*)best_idx);
}
agp_status agp_pathwise_info(agp_pathwise* p, int32_t* n_latent, int32_t* n_features, int32_t* n_samples, int64_t* m, int64_t* D) {
  if (!p) return AGP_ERR_INVALID;
  if (n_latent) *n_latent = p->nl;
  if (n_features) *n_features = p->L;
  if (n_samples) *n_samples = p->S;
  if (m) *m = p->m;
  if (D) *D = p->D;
  return AGP_OK;
}
agp_status agp_pathwise_get(agp_pathwise* p, int32_t latent, int32_t which, void* out, int64_t ld) {
  if (!p) return AGP_ERR_INVALID;
  agp_ctx* ctx = p->ctx;
  if (latent < 0 || latent >= p->nl || !out || which < AGP_PW_OMEGA || which > AGP_PW_E) {
    ctx->err = "agp_pathwise_get: latent in [0, n_latent), out given, which one of AGP_PW_OMEGA .. AGP_PW_E";
    return AGP_ERR_INVALID;
  }
  const agp_pathwise::Lat& a = p->lat[latent];
  const double* src = a.omega;
  int64_t sr = p->D, sc = 1, rows = p->L, cols = p->D;
  switch (which) {
    case AGP_PW_PHASE: src = a.phase, sr = 1, cols = 1, ld = 1; break;  // a dense vector: ld is not read
    case AGP_PW_W: src = a.WV, sr = 1, sc = p->ldw, cols = p->S; break;
    case AGP_PW_V: src = a.WV + p->Lp, sr = 1, sc = p->ldw, rows = p->m, cols = p->S; break;
    case AGP_PW_E: src = a.E, sr = p->Sp, rows = p->m, cols = p->S; break;
    default: break;
  }
  if (ld < cols) {
    ctx->err = "agp_pathwise_get: the leading dimension is smaller than the table's width (" + std::to_string(cols) + ")";
    return AGP_ERR_INVALID;
  }
  DevGuard guard(ctx->device);
  hipLaunchKernelGGL(k_pw_gather, grid2(rows, cols), blk2, 0, ctx->stream, src, sr, sc, rows, cols, (double*)out, ld);
  LAUNCHCHK(ctx);
  return AGP_OK;
}
agp_status agp_pathwise_destroy(agp_pathwise* p) {
  if (!p) return AGP_OK;
  DevGuard guard(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  delete p;
  return AGP_OK;
}
agp_status agp_pathwise_features(agp_ctx* ctx, const agp_kernel_desc* k, int64_t D, int32_t n_features, uint64_t seed, int64_t t,
                                 int32_t latent, void* omega_out, void* phase_out) {
  if (!ctx) return AGP_ERR_INVALID;
  if (!k || !omega_out || !phase_out || k->kind < AGP_K_SQEXP || k->kind > AGP_K_EXPONENTIAL || latent < 0 || latent > (1 << 24)) {
    ctx->err = "agp_pathwise_features: k, omega_out and phase_out must be given, k->kind one of the four kernels, latent >= 0";
    return AGP_ERR_INVALID;
  }
  AGPCHK(pw_check_spectral(ctx, "agp_pathwise_features", D, n_features, t));
  DevGuard guard(ctx->device);
  AGPCHK(pw_spectral(ctx, k->kind, D, n_features, seed, t, latent, (double*)omega_out, (double*)phase_out));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

agp_status agp_svgp_set_online_prior(agp_svgp* h, int32_t latent, const void* za, int64_t ldza, int64_t ma, const void* invDa,
                                     int64_t ldi, const void* prev_eta1, double prevLa) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_set_online_prior");
  return h->impl->set_online_prior(latent, za, ldza, ma, invDa, ldi, prev_eta1, prevLa);
}
agp_status agp_svgp_online_snapshot(agp_svgp* h, int32_t latent, void* invDa_out, int64_t ldi, void* eta1_out,
                                    double* prevLa_host) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_online_snapshot");
  return h->impl->online_snapshot(latent, invDa_out, ldi, eta1_out, prevLa_host);
}
agp_status agp_svgp_adopt_local(agp_svgp* dst, agp_svgp* src) {
  HCHKF(dst);
  FULLNO(dst, "agp_svgp_adopt_local");
  if (!src || !src->impl) return AGP_ERR_INVALID;
  AGPCHK(src->impl->flush());
  return dst->impl->adopt_local(src->impl);
}
agp_status agp_svgp_online_first_step(agp_svgp* h_new, agp_svgp* h_old, const void* x, int64_t ldx, const void* y,
                                      int64_t B) {
  HCHKF(h_new);
  FULLNO(h_new, "agp_svgp_online_first_step");
  if (!h_old || !h_old->impl) return AGP_ERR_INVALID;
  AGPCHK(h_old->impl->flush());
  SvgpBase *n = h_new->impl, *o = h_old->impl;
  // local update of the new batch under the OLD inducing points and posterior (compute_old_matrices, onlinetraining.jl:80-89)
  AGPCHK(o->step_local(x, ldx, y, nullptr, B, 1.0, true));
  if (o->desc.lik.kind == AGP_LIK_LOGISTICSOFTMAX) {
    for (int it = 0; it < 2; ++it) {
      AGPCHK(o->lsm_gamma());
      AGPCHK(o->lsm_alpha());
    }
  }
  // kernel matrices of the new inducing points, then the online natural gradient with those expectation gradients (:93-104)
  AGPCHK(n->step_local(x, ldx, y, nullptr, B, 1.0, true));
  AGPCHK(n->adopt_local(o));
  AGPCHK(n->step_stats(true));
  return n->step_global(true);
}

agp_status agp_svgp_hyper_apply(agp_svgp* h, int32_t latent, const double* dvariance_host, const double* dscale_host,
                                const void* dZ) {
  HCHKF(h);
  if (dZ) FULLNO(h, "a dZ gradient");
  return h->impl->hyper_apply(latent, dvariance_host, dscale_host, dZ);
}
agp_status agp_svgp_hyper_opt_state(agp_svgp* h, int32_t latent, int32_t set, double* k_m_host, double* k_v_host,
                                    int32_t* k_step_host) {
  HCHKF(h);
  return h->impl->hyper_state(latent, set, k_m_host, k_v_host, k_step_host);
}
agp_status agp_svgp_set_quadrature(agp_svgp* h, const double* gh_nodes_host, const double* gh_weights_host,
                                   int32_t n_nodes) {
  HCHKF(h);
  return h->impl->set_quadrature(gh_nodes_host, gh_weights_host, n_nodes);
}
agp_status agp_svgp_set_lsm_alpha(agp_svgp* h, const void* alpha, int64_t n) {
  HCHKF(h);
  return h->impl->set_lsm_alpha(alpha, n);
}
agp_status agp_svgp_get_lik_param(agp_svgp* h, double* out) {
  HCHKF(h);
  return h->impl->get_lik_param(out);
}
agp_status agp_svgp_set_lik_param(agp_svgp* h, double value) {
  HCHKF(h);
  return h->impl->set_lik_param(value);
}


// ---- collectives (agp_comm.h) ------------------------------------------------------------------------------------
agp_status agp_comm_unique_id(uint8_t* id_host) {
  if (!id_host) return AGP_ERR_INVALID;
  std::string why;
  RcclApi* api = rccl_api(why);
  if (!api) return AGP_ERR_UNSUPPORTED;
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return AGP_ERR_HIP;
  static_assert(sizeof(id) == AGP_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(id_host, &id, sizeof(id));
  return AGP_OK;
}

agp_status agp_comm_init(agp_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id_host, agp_comm** out) {
  if (!ctx || !out || !id_host || world < 1 || rank < 0 || rank >= world) return AGP_ERR_INVALID;
  *out = nullptr;
  DevGuard guard(ctx->device);
  std::string why;
  RcclApi* api = rccl_api(why);
  if (!api) {
    ctx->err = "agp_comm_init: " + why;
    return AGP_ERR_UNSUPPORTED;
  }
  ncclUniqueId id;
  memcpy(&id, id_host, sizeof(id));
  ncclComm_t c = nullptr;
  ncclResult_t r = api->CommInitRank(&c, world, id, rank);  // binds to the current device = ctx->device
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclCommInitRank : ") + api->GetErrorString(r) + " [" + api->where + "]";
    return AGP_ERR_HIP;
  }
  agp_comm* cm = new agp_comm();
  cm->ctx = ctx;
  cm->rank = rank;
  cm->world = world;
  cm->kind = 0;
  cm->nccl = c;
  *out = cm;
  return AGP_OK;
}

agp_status agp_comm_init_callback(agp_ctx* ctx, int32_t rank, int32_t world, agp_allreduce_fn fn, void* user,
                                  agp_comm** out) {
  if (!ctx || !out || !fn || world < 1 || rank < 0 || rank >= world) return AGP_ERR_INVALID;
  agp_comm* cm = new agp_comm();
  cm->ctx = ctx;
  cm->rank = rank;
  cm->world = world;
  cm->kind = 1;
  cm->fn = fn;
  cm->user = user;
  *out = cm;
  return AGP_OK;
}

agp_status agp_comm_destroy(agp_comm* cm) {
  if (!cm) return AGP_OK;
  DevGuard guard(cm->ctx->device);
  (void)hipStreamSynchronize(cm->ctx->stream);
  for (auto e : cm->ev) (void)hipEventDestroy(e);
  if (cm->side) {
    (void)hipStreamSynchronize(cm->side);
    (void)hipStreamDestroy(cm->side);
  }
  if (cm->ev_in) (void)hipEventDestroy(cm->ev_in);
  if (cm->ev_out) (void)hipEventDestroy(cm->ev_out);
  if (cm->kind == 0 && cm->nccl) {
    std::string why;
    RcclApi* api = rccl_api(why);
    if (api) (void)api->CommDestroy(cm->nccl);
  }
  delete cm;
  return AGP_OK;
}

agp_status agp_comm_info(agp_comm* cm, int32_t* rank_host, int32_t* world_host, int32_t* is_rccl_host) {
  if (!cm) return AGP_ERR_INVALID;
  if (rank_host) *rank_host = cm->rank;
  if (world_host) *world_host = cm->world;
  if (is_rccl_host) *is_rccl_host = cm->kind == 0;
  return AGP_OK;
}

}  // extern "C"

#include "agp_comm_host.h"

extern "C" {

agp_status agp_comm_standin_allreduce(void* buf, int64_t count, int32_t dtype, void* stream, int32_t n_wg, int32_t n_threads,
                                      double min_us, int32_t* stuck_dev) {
  if (!buf || count <= 0 || (dtype != AGP_F64 && dtype != AGP_F32) || n_wg < 1 || n_wg > 64 || n_threads < 64 || n_threads > 1024)
    return AGP_ERR_INVALID;
  const int64_t n8 = count * (dtype == AGP_F64 ? 8 : 4) / 8;  // whole 8-byte words (a trailing float stays where it is)
  const unsigned long long base = g_standin_launches * 2ull * (unsigned long long)n_wg;
  // (the counter's base assumes one n_wg per process: the stand-in is a diagnostic of ONE configuration per run)
  g_standin_launches += 1;
  hipLaunchKernelGGL(k_standin_allreduce, dim3((unsigned)n_wg), dim3((unsigned)n_threads), 0, (hipStream_t)stream,
                     (unsigned long long*)buf, n8, base, min_us, stuck_dev);
  return hipGetLastError() == hipSuccess ? AGP_OK : AGP_ERR_HIP;
}

agp_status agp_comm_allreduce(agp_comm* cm, void* buf, int64_t count, int32_t dtype) {
  if (!cm || !buf || count <= 0 || (dtype != AGP_F64 && dtype != AGP_F32)) return AGP_ERR_INVALID;
  agp_ctx* ctx = cm->ctx;
  DevGuard guard(ctx->device);
  cm->n_calls += 1;
  cm->bytes += count * (dtype == AGP_F64 ? 8 : 4);
  AGPCHK(comm_timing_begin(cm, ctx->stream));
  AGPCHK(comm_issue(cm, buf, count, dtype, ctx->stream));
  return comm_timing_end(cm, ctx->stream);
}

agp_status agp_comm_timing(agp_comm* cm, int32_t on) {
  if (!cm) return AGP_ERR_INVALID;
  cm->timing = on != 0;
  cm->timing_every = on > 1 ? on : 1;
  return AGP_OK;
}

agp_status agp_comm_stats(agp_comm* cm, int64_t* n_calls_host, int64_t* bytes_host, double* ms_host) {
  if (!cm) return AGP_ERR_INVALID;
  agp_ctx* ctx = cm->ctx;
  DevGuard guard(ctx->device);
  if (n_calls_host) *n_calls_host = cm->n_calls;
  if (bytes_host) *bytes_host = cm->bytes;
  double ms = 0.0;
  if (cm->ev_used) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (cm->side) HIPCHK(ctx, hipStreamSynchronize(cm->side));
    for (size_t i = 0; i + 1 < cm->ev_used; i += 2) {
      float t = 0;
      HIPCHK(ctx, hipEventElapsedTime(&t, cm->ev[i], cm->ev[i + 1]));
      ms += t;
    }
  }
  // with every n-th collective bracketed the sum is scaled to all of them
  if (cm->n_timed > 0 && cm->n_timed < cm->n_calls) ms *= (double)cm->n_calls / (double)cm->n_timed;
  if (ms_host) *ms_host = ms;
  cm->n_calls = cm->bytes = 0;
  cm->n_timed = 0;
  cm->ev_used = 0;
  return AGP_OK;
}

agp_status agp_svgp_cavi_step_multi(agp_svgp* h, agp_comm* comm, int32_t mode, const void* x, int64_t ldx, const void* y,
                                    const int64_t* idx, int64_t B, double rho) {
  HCHK(h);  // (no flush: like agp_svgp_cavi_step, the step takes a pending natural-gradient step itself -- as its prologue)
  FULLNO(h, "agp_svgp_cavi_step_multi");
  h->impl->n_steps += 1;
  return h->impl->cavi_step_multi(comm, mode, x, ldx, y, idx, B, rho);
}
agp_status agp_svgp_elbo_multi(agp_svgp* h, agp_comm* comm, int32_t mode, double* elbo_host) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_elbo_multi");
  return h->impl->elbo_multi(comm, mode, elbo_host);
}
agp_status agp_svgp_hyper_step_multi(agp_svgp* h, agp_comm* comm, int32_t tied) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_hyper_step_multi");
  return h->impl->hyper_step_multi(comm, tied);
}
agp_status agp_svgp_predict_multi(agp_svgp* h, agp_comm* comm, int32_t what, const void* xt, int64_t ldx, int64_t n_t,
                                  void* mu_out, void* var_out, const double* gh_nodes_host, const double* gh_weights_host,
                                  int32_t n_nodes) {
  HCHKF(h);
  FULLNO(h, "agp_svgp_predict_multi");
  if (n_t == 0) return AGP_OK;  // no test points: nothing to write (the reference returns empty arrays)
  return h->impl->predict_multi(comm, what, xt, ldx, n_t, mu_out, var_out, gh_nodes_host, gh_weights_host, n_nodes);
}

agp_status agp_svgp_proba_y(agp_svgp* h, const void* xt, int64_t ldx, int64_t n_t, const double* gh_nodes_host,
                            const double* gh_weights_host, int32_t n_nodes, void* out0, void* out1) {
  HCHKF(h);
  if (n_t == 0) return AGP_OK;  // no test points: nothing to write (the reference returns empty arrays)
  return h->impl->proba_y(xt, ldx, n_t, gh_nodes_host, gh_weights_host, n_nodes, out0, out1);
}

}  // extern "C"
