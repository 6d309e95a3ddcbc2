// agp_svgp_base.h -- SvgpBase, the type-erased interface every model handle of the C ABI is called through (struct agp_svgp holds
// one), with what all classes share: the streamed log predictive density (lpd_stream; host driver agp_lpd_host.h, kernels
// agp_lpd.h), the refusals by name, the step counters and the HIP-event timing.  Also here: KernelHost (the host's copy of a kernel
// object), k_elbo_combine (the last line of the enqueued ELBO, the one kernel of this header) and the teardown helpers dcheck /
// dfree.  The classes behind the interface: Svgp<T> and what derives from it (Vgp, Movgp, Gp, Mcgp, Nvgp, Nsvgp), all in
// agp_capi.hip.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "agp_comm.h"
#include "agp_ctx.h"
#include "agp_lpd.h"
#include "agp_lpd_host.h"

static agp_status comm_allreduce_groups(agp_comm* cm, void* base, int esz, const int64_t* off, const int64_t* cnt, int ng,
                                        int32_t dtype, int32_t* arrive, int32_t epoch);  // (defined in agp_comm_host.h)

// ---- model ---------------------------------------------------------------------------------------------------
struct KernelHost {
  int kind = AGP_K_SQEXP;
  double variance = 1.0;
  bool ard = false;
  bool has_variance = true, has_transform = true;  // structure of the kernel object (agp_kernel_desc): what update_kernel! steps
  std::vector<double> scales;  // length D
};

namespace agp {
struct AcqParams;  // agp_acq.h
}
struct AcqModel;  // agp_acq_host.h
struct AcqDriver;
struct AcqJointDriver;  // agp_acq_joint_host.h

struct SvgpBase {
  agp_ctx* ctx = nullptr;
  agp_svgp_desc desc{};
  virtual ~SvgpBase() {
    for (void* p : {lpd_mu, lpd_var, (void*)lpd_part, (void*)lpd_scal})
      if (p) (void)hipFree(p);
  }
  virtual agp_status init() = 0;
  virtual agp_status set_kernel(int l, const agp_kernel_desc* k) = 0;
  virtual agp_status set_Z(int l, const void* z, int64_t ldz) = 0;
  virtual agp_status get_Z(int l, void* z, int64_t ldz) = 0;
  virtual agp_status set_mu0(int l, const void* mu0) = 0;
  virtual agp_status refresh_K() = 0;
  virtual agp_status step_local(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho,
                                bool fresh) = 0;
  virtual agp_status prefetch(const void* x, int64_t ldx, const int64_t* idx, int64_t B) = 0;
  virtual agp_status set_multioutput(int n_task, const agp_lik_desc* liks, const double* A_host, double eta, double b1,
                                     double b2, double eps) = 0;
  virtual agp_status get_A(double* A_host) = 0;
  virtual agp_status mo_shard(int q_total) = 0;
  virtual agp_status mo_fbuf_ptr(void** p, int64_t* n) = 0;
  virtual agp_status mo_mix() = 0;
  virtual agp_status mo_refresh_f() = 0;
  virtual agp_status mo_predict_from_f(int64_t nt, int mode, void* o0, void* o1, const double* nodes,
                                       const double* weights, int nn) = 0;
  virtual agp_status hyper_rule(int k_rule, double k_rho, int z_rule, double z_rho) = 0;
  virtual agp_status hyper_configure(int opt_k, double k_eta, int opt_z, double z_eta, double b1, double b2,
                                     double eps) = 0;
  virtual agp_status hypergrad(int l, double* dvar, double* dscale, void* dZ) = 0;
  virtual agp_status hyper_step() = 0;
  virtual agp_status get_kernel(int l, double* var, double* scales) = 0;
  virtual agp_status lsm_gamma() = 0;
  virtual agp_status lsm_alpha() = 0;
  virtual agp_status lsm_local_all() = 0;  // both rounds and the final theta, r, w of a handle holding every latent
  virtual agp_status lsm_gsum_ptr(void** p, int64_t* n) = 0;
  virtual agp_status step_stats(bool fused) = 0;
  virtual agp_status stats_ptr(void** p, int64_t* n) = 0;
#ifdef AGP_DEBUG_PTRS  // (development builds only: device addresses of the step's state, tools/tmp)
  virtual void* debug_ptr(int what) { (void)what; return nullptr; }
#endif
  virtual agp_status step_global(bool fused) = 0;
  // tail of agp_svgp_cavi_step: the fused natural-gradient step now, or left pending for the next step's task-graph launch
  virtual agp_status step_finish() = 0;
  // applies a pending natural-gradient step with the stand-alone kernel (every entry point other than the CAVI step calls this
  // first, so eta, Sigma, predictions, the ELBO and the hyper-gradient never see a half-taken step)
  virtual agp_status flush() = 0;
  virtual agp_status check_status() = 0;
  virtual agp_status elbo(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho,
                          int fresh, double* out) = 0;
  virtual agp_status elbo_terms(double* out3) = 0;
  // streamed full-data ELBO ("STREAMED ELBO"): sparse AnalyticVI / AnalyticSVI handles evaluate (Svgp<T>); every other class
  // refuses by name before anything is launched
  agp_status elbo_stream_refused(const char* why) {
    ctx->err = std::string("agp_svgp_elbo_stream: ") + why;
    return AGP_ERR_UNSUPPORTED;
  }
  virtual agp_status elbo_stream(const void*, int64_t, const void*, const int64_t*, int64_t, double, double*, double*) {
    return elbo_stream_refused("this handle class has no streamed ELBO (sparse AnalyticVI / AnalyticSVI handles only)");
  }
  // ---- streamed log predictive density (include/agp_hip.h, "LOG PREDICTIVE DENSITY") ------------------------
  // sum_i log p(y_i | x_i, model) over any number of points: the handle's own predict_f, chunk by chunk, leaves the moments of 4096
  // points in lpd_mu / lpd_var; k_predict_lpd turns them into one partial sum per workgroup; k_lpd_reduce adds all of them in a
  // fixed order.  One routine for every class whose predict_f works.  Touches the predictor's workspace and the buffers below --
  // never step buffers, local variables, caches or status words.  One synchronisation, at the end.
  void *lpd_mu = nullptr, *lpd_var = nullptr;  // T[n_latent][4096]
  double* lpd_part = nullptr;                  // one per workgroup of the stream
  int64_t lpd_part_cap = 0;
  double* lpd_scal = nullptr;                  // out[3] of k_lpd_reduce | - | the two failure words
  LpdRule lpd_rule;
  // what the routine has to ask the class: the likelihood-state word on the device (Gaussian noise under opt_noise, Poisson lambda;
  // NULL: the descriptor's p0 holds), and whether the handle sees a shard of every minibatch
  virtual const void* lpd_lik_state() { return nullptr; }
  virtual bool lpd_batch_sharded() { return false; }
  agp_status lpd_refused(const char* why) {
    ctx->err = std::string("agp_svgp_lpd_stream: ") + why;
    return AGP_ERR_UNSUPPORTED;
  }
  agp_status lpd_stream(const void* xt, int64_t ldx, const void* y, int64_t n, const double* nodes, const double* weights, int nn,
                        double* sum_host, void* lpd_out) {
    const int kind = desc.lik.kind;
    if (desc.flags & AGP_FLAG_SAMPLED)
      return lpd_refused("Gibbs-sampled models (AGP_FLAG_SAMPLED) are not supported: they have no predict_f");
    if (kind == AGP_LIK_MULTIOUTPUT) return lpd_refused("multi-output handles (AGP_LIK_MULTIOUTPUT) are not supported");
    if (kind == AGP_LIK_HETEROSCEDASTIC)
      return lpd_refused("Heteroscedastic is not supported (two latents, a nested integral: a follow-up)");
    if (!lpd_lik_ok(kind)) return lpd_refused("unknown likelihood kind");
    if (desc.latent_offset != 0 || desc.n_latent != (lpd_is_multiclass(kind) ? desc.lik.n_class : 1))
      return lpd_refused("latent-sharded handles are not supported (a point's density needs every latent on one handle)");
    if (lpd_batch_sharded()) return lpd_refused("batch-sharded handles are not supported");
    if (n < 0 || !sum_host || (n > 0 && (!xt || !y || ldx < desc.D))) {
      ctx->err = "agp_svgp_lpd_stream: n >= 0, sum_host must not be NULL, x and y must not be NULL, ldx >= D";
      return AGP_ERR_INVALID;
    }
    if (n == 0) {
      *sum_host = 0.0;
      return AGP_OK;
    }
    return desc.dtype == AGP_F32 ? lpd_stream_t<float>(xt, ldx, y, n, nodes, weights, nn, sum_host, lpd_out)
                                 : lpd_stream_t<double>(xt, ldx, y, n, nodes, weights, nn, sum_host, lpd_out);
  }
  template <typename T>
  agp_status lpd_stream_t(const void* xt, int64_t ldx, const void* y, int64_t n, const double* nodes, const double* weights, int nn,
                          double* sum_host, void* lpd_out) {
    const char* who = "agp_svgp_lpd_stream";
    const int kind = desc.lik.kind, nl = desc.n_latent;
    const int64_t CH = 4096, ppb = lpd_points_per_block(kind);
    const int64_t nw = (n + ppb - 1) / ppb;
    hipStream_t s = ctx->stream;
    LpdParams P;
    AGPCHK(lpd_params(ctx, who, desc.lik, &P));
    if (lpd_is_quad(kind)) AGPCHK(lpd_rule.ensure(ctx, who, s, nodes, weights, nn));
    if (!lpd_mu) {
      AGPCHK(dmalloc(ctx, (T**)&lpd_mu, (int64_t)nl * CH));
      AGPCHK(dmalloc(ctx, (T**)&lpd_var, (int64_t)nl * CH));
      AGPCHK(dmalloc(ctx, &lpd_scal, 8));
    }
    if (nw > lpd_part_cap) {
      if (lpd_part) (void)hipFree(lpd_part);
      lpd_part = nullptr;
      lpd_part_cap = 0;
      AGPCHK(dmalloc(ctx, &lpd_part, nw));
      lpd_part_cap = nw;
    }
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(lpd_scal + 4);
    HIPCHK(ctx, hipMemsetAsync(bad, 0xFF, 2 * sizeof(unsigned long long), s));
    const T* lstate = (const T*)lpd_lik_state();
    for (int64_t st0 = 0; st0 < n; st0 += CH) {
      const int64_t nc = (n - st0) < CH ? (n - st0) : CH;
      AGPCHK(predict_f((const T*)xt + st0 * ldx, ldx, nc, lpd_mu, lpd_var));  // T[nl][nc]
      AGPCHK(lpd_launch<T>(ctx, s, kind, nc, st0, nl, nc, P, lstate, y, (const T*)lpd_mu, (const T*)lpd_var, lpd_rule.dev, nn,
                           (T*)lpd_out, lpd_part + st0 / ppb, bad));
    }
    hipLaunchKernelGGL(k_lpd_reduce, dim3(1), dim3(1024), 0, s, (const double*)lpd_part, nw, (const unsigned long long*)bad, lpd_scal);
    LAUNCHCHK(ctx);
    double h[3] = {0.0, -1.0, -1.0};
    HIPCHK(ctx, hipMemcpyAsync(h, lpd_scal, sizeof(double) * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    AGPCHK(lpd_failure(ctx, who, h));
    *sum_host = h[0];
    return AGP_OK;
  }
  virtual agp_status elbo_enqueue(const void* x, int64_t ldx, const void* y, const int64_t* idx, int64_t B, double rho, int fresh,
                                  int32_t* ticket) = 0;
  virtual agp_status elbo_fetch(int32_t ticket, int wait, double* out, int32_t* ready) = 0;
  virtual agp_status set_batch_shard(int rank, int world) = 0;
  virtual agp_status get_state(int l, void* mu, void* sigma, void* eta1, void* eta2) = 0;
  virtual agp_status set_state(int l, const void* eta1, const void* eta2) = 0;
  virtual agp_status get_matrix(int l, int which, void* out, int64_t ldo, int64_t cap) = 0;
  virtual int64_t last_batch() = 0;
  virtual agp_status init_state() = 0;
  virtual agp_status invalidate_data() = 0;
  virtual agp_status predict_f_cov(const void* xt, int64_t ldx, int64_t nt, void* mu, void* cov) = 0;
  virtual agp_status refresh_K_explicit() = 0;
  // multi-GPU (agp_comm.h)
  virtual agp_status cavi_step_multi(agp_comm* cm, int mode, const void* x, int64_t ldx, const void* y, const int64_t* idx,
                                     int64_t B, double rho) = 0;
  virtual agp_status elbo_multi(agp_comm* cm, int mode, double* out) = 0;
  virtual agp_status hyper_step_multi(agp_comm* cm, int tied) = 0;
  virtual agp_status predict_multi(agp_comm* cm, int what, const void* xt, int64_t ldx, int64_t nt, void* mu, void* var,
                                   const double* nodes, const double* weights, int nn) = 0;
  virtual agp_status predict_f(const void* xt, int64_t ldx, int64_t nt, void* mu, void* var) = 0;
  // input gradients of the predictive moments ("PREDICTIVE GRADIENTS"; Svgp<T>::predict_f_grad serves every class)
  virtual agp_status predict_f_grad(const void* xt, int64_t ldx, int64_t nt, void* dmu, void* dvar, int64_t ldg) = 0;
  // acquisition functions of one latent ("ACQUISITION FUNCTIONS"): AcqDriver / AcqJointDriver (agp_acq_host.h, agp_acq_joint_host.h)
  // serve every class and ask the handle two things.  acq_check refuses, for the entry point `who`, the handles, descriptors, latents
  // and kernels that have no acquisition function, and touches nothing; acq_open readies the predictor of latent l and the chunk
  // workspaces (with those of an ascent), and hands out its view of them and the handle's drivers.  Also here: the predictor's two
  // objects (AGP_VEC_APRED / AGP_MAT_APRED of agp_svgp_get_matrix)
  virtual agp_status acq_check(const char* who, int l, const agp_acq_desc* d, agp::AcqParams* p) = 0;
  virtual agp_status acq_open(int l, bool ascent, AcqModel* model, AcqDriver** plain, AcqJointDriver** joint) = 0;
  virtual agp_status get_predictor(int l, int which, void* out, int64_t ldo, int64_t cap) = 0;
  virtual agp_status predict_y(const void* xt, int64_t ldx, int64_t nt, void* out) = 0;
  virtual agp_status proba_y(const void* xt, int64_t ldx, int64_t nt, const double* nodes, const double* weights,
                             int nn, void* o0, void* o1) = 0;
  virtual agp_status set_quadrature(const double* nodes, const double* weights, int nn) = 0;
  virtual agp_status hyper_state(int l, int set, double* k_m, double* k_v, int32_t* k_step) = 0;
  virtual agp_status hyper_apply(int l, const double* dvar, const double* dscale, const void* dZ) = 0;
  virtual agp_status set_lsm_alpha(const void* a, int64_t n) = 0;
  virtual agp_status set_online_prior(int l, const void* za, int64_t ldza, int64_t ma, const void* invDa, int64_t ldi,
                                      const void* peta1, double prevLa) = 0;
  virtual agp_status online_snapshot(int l, void* invDa_out, int64_t ldi, void* eta1_out, double* prevLa_host) = 0;
  virtual agp_status adopt_local(SvgpBase* src) = 0;
  virtual agp_status get_lik_param(double* out) = 0;
  virtual agp_status set_lik_param(double v) = 0;
  // Gibbs sampling (AGP_FLAG_SAMPLED: Mcgp); every other handle refuses
  agp_status not_sampled(const char* what) {
    ctx->err = std::string(what) + ": the handle is not a Gibbs-sampled model (AGP_FLAG_FULL | AGP_FLAG_SAMPLED)";
    return AGP_ERR_UNSUPPORTED;
  }
  virtual agp_status gibbs_sample(const void*, int64_t, int64_t, int64_t, uint64_t, void*, int64_t) {
    return not_sampled("agp_svgp_gibbs_sample");
  }
  virtual agp_status gibbs_counter(int, int64_t*) { return not_sampled("agp_svgp_gibbs_counter"); }
  virtual agp_status predict_samples(const void*, int64_t, int64_t, const void*, int64_t, int64_t, int, void*, void*) {
    return not_sampled("agp_svgp_predict_samples");
  }
  // numerical inference (AGP_FLAG_NUMERICAL: Nvgp, Nsvgp); every other handle refuses
  agp_status not_numerical(const char* what) {
    ctx->err = std::string(what) + ": the handle does not run numerical inference (AGP_FLAG_NUMERICAL, with or without AGP_FLAG_FULL)";
    return AGP_ERR_UNSUPPORTED;
  }
  virtual agp_status nvi_configure(int, const double*, const double*, int, int, double, double, double, double) {
    return not_numerical("agp_svgp_nvi_configure");
  }
  virtual agp_status mcvi_configure(int, uint64_t, int, int, double, double, double, double) {
    return not_numerical("agp_svgp_mcvi_configure");
  }
  virtual agp_status nvi_step(const void*, int64_t, const void*, const int64_t*, int64_t, double) {
    return not_numerical("agp_svgp_nvi_step");
  }
  virtual agp_status nvi_info(int, double*, int64_t*, int64_t*) { return not_numerical("agp_svgp_nvi_info"); }
  virtual agp_status nvi_state(int, int, void*, void*, int64_t*) { return not_numerical("agp_svgp_nvi_state"); }
  // pathwise sampling ("PATHWISE SAMPLING"): Svgp<double>, Vgp and Gp draw; every other class refuses by name
  virtual agp_status pathwise_draw(int n_features, int n_samples, uint64_t seed, int64_t t, agp_pathwise** out) = 0;
  agp_status pathwise_refused(const char* why) {
    ctx->err = std::string("agp_svgp_pathwise_draw: ") + why;
    return AGP_ERR_UNSUPPORTED;
  }
  int64_t n_opt = 1;  // RobbinsMonro counter (optimisers.jl:12)
  bool in_cavi_step = false;  // step_local is running as the first half of agp_svgp_cavi_step (its tail may then be deferred)
  int64_t n_prologue = 0;  // CAVI steps whose natural-gradient part rode on the next step's task-graph launch (agp_svgp_step_counters)
  int64_t n_steps = 0;     // agp_svgp_cavi_step calls
  int64_t n_hgrad = 0, n_gk_fused = 0;  // hyper-gradient evaluations / those with the one-product G_K (agp_svgp_hyper_counters)
  // HIP-event timing of the dominant kernel sequence (agp_svgp_timing_*)
  bool timing = false;
  int timing_every = 1, timing_ctr = 0;  // every n-th sequence is bracketed (the two event records cost the step ~16 us at C2)
  bool timing_now = false;
  std::vector<hipEvent_t> ev;
  std::vector<int64_t> ev_launches;
  size_t ev_used = 0;
  agp_status timing_begin() {
    timing_now = timing && (timing_ctr++ % timing_every) == 0;
    if (!timing_now) return AGP_OK;
    if (ev_used + 2 > ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreate(&e));
        ev.push_back(e);
      }
    }
    HIPCHK(ctx, hipEventRecord(ev[ev_used], ctx->stream));
    return AGP_OK;
  }
  agp_status timing_end(int64_t launches) {
    if (!timing_now) return AGP_OK;
    timing_now = false;
    HIPCHK(ctx, hipEventRecord(ev[ev_used + 1], ctx->stream));
    ev_used += 2;
    ev_launches.push_back(launches);
    return AGP_OK;
  }
  agp_status timing_read(int64_t* n, double* ms) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *n = 0;
    *ms = 0.0;
    for (size_t i = 0; i + 1 < ev_used; i += 2) {
      float t = 0;
      HIPCHK(ctx, hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      *ms += t;
      *n += ev_launches[i / 2];
    }
    ev_used = 0;
    ev_launches.clear();
    return AGP_OK;
  }
};

// the last line of the ELBO on the device (agp_svgp_elbo_enqueue): rho E_data - KL(q(u) || p(u)) - rho KL_aug from the five partial
// results of the evaluation and log det K, written to mapped host memory -- no stream synchronisation on the host's side
__global__ void k_elbo_combine(const double* __restrict__ sc, const double* __restrict__ half_logdetK, double m, double rho,
                               double* __restrict__ out) {
  const double kl = 0.5 * (2.0 * half_logdetK[0] + 2.0 * sc[2] + sc[3] + sc[4] - m);  // log det Sigma = -2 sc[2]
  *out = rho * sc[0] - kl - rho * sc[1];
  __threadfence_system();
}

struct agp_svgp {
  SvgpBase* impl;
};

// teardown helpers: a failing free / destroy is a bug in this library, so it is reported, never swallowed
static void dcheck(hipError_t e, const char* file, int line) {
  if (e != hipSuccess) fprintf(stderr, "[agp_hip] teardown: %s (%s:%d)\n", hipGetErrorString(e), file, line);
}
#define dfree(p) dcheck(hipFree(p), __FILE_NAME__, __LINE__)
