// agp_acq_host.h -- host driver of the acquisition functions (kernels: agp_acq.h; include/agp_hip.h "ACQUISITION FUNCTIONS"): the
// argument checks of agp_acq_desc and agp_pw_ascent_opts, which touch nothing, agp_acq_moments, the launch of k_acq_contract and the
// particle state of the ascent, and AcqDriver, which drives all the launches of agp_svgp_acquisition, agp_svgp_acq_maximize and the
// two calls with pending points.  It is Float64 code that reads the model through AcqModel, the view of one latent's predictor that
// the handle fills (SvgpBase::acq_open; Svgp<T> in agp_capi.hip), and writes nothing of the model's.
// Batch acquisition (kernels: agp_acq_batch.h): AcqPred names the predictor a pass runs on -- the latent's own objects, or the
// augmented ones of AcqBatchWs, which the bordering launches below extend by one pending point at a time.
#pragma once
#include <cmath>
#include <string>

#include "agp_acq.h"
#include "agp_acq_batch.h"
#include "agp_acq_check.h"
#include "agp_blas_host.h"  // kmm_usable, kmm_dp, launch_kernelmatrix, gemm_nt
#include "agp_ctx.h"
#include "agp_svgp_base.h"

// desc -> AcqParams, or AGP_ERR_INVALID with a message
static agp_status acq_check_desc(agp_ctx* ctx, const char* who, const agp_acq_desc* d, agp::AcqParams* out) {
  auto invalid = [&](const std::string& what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (!d) return invalid("desc must be given");
  if (d->kind != AGP_ACQ_UCB && d->kind != AGP_ACQ_EI && d->kind != AGP_ACQ_PI && d->kind != AGP_ACQ_LOG_EI && d->kind != AGP_ACQ_LOG_PI)
    return invalid("unknown kind (AGP_ACQ_UCB, AGP_ACQ_EI, AGP_ACQ_PI, AGP_ACQ_LOG_EI or AGP_ACQ_LOG_PI)");
  if (!std::isfinite(d->beta) || !std::isfinite(d->best) || !std::isfinite(d->xi)) return invalid("beta, best and xi must be finite");
  if (d->beta < 0.0) return invalid("beta >= 0");
  if (d->xi < 0.0) return invalid("xi >= 0");
  out->kind = d->kind;
  out->s = d->minimize ? -1.0 : 1.0;
  out->beta = d->beta, out->best = d->best, out->xi = d->xi;
  return AGP_OK;
}

// the checks of agp_pathwise_maximize on the options it shares (pw_maximize), in its words; the direction and the shared starts
// belong to the paths and must be 0 here
static agp_status acq_check_opts(agp_ctx* ctx, const char* who, int64_t D, const agp_pw_ascent_opts* o, agp::PwAscentBox* box) {
  auto invalid = [&](const std::string& what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (!o) return invalid("opts must be given");
  if (o->minimize != 0 || o->x0_shared != 0) return invalid("opts->minimize and opts->x0_shared must be 0 (the direction is agp_acq_desc.minimize)");
  if (o->steps < 0 || o->steps > 65536) return invalid("steps must lie in [0, 65536]");
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return invalid("0 <= beta1, beta2 < 1");
  if (!(o->eps > 0.0) || !std::isfinite(o->eps)) return invalid("eps must be finite and > 0");
  if (!o->lo_host || !o->hi_host || !o->lr_host) return invalid("lo_host, hi_host and lr_host must be given");
  *box = agp::PwAscentBox{};
  for (int64_t d = 0; d < D; ++d) {
    const double lo = o->lo_host[d], hi = o->hi_host[d], lr = o->lr_host[d];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi))
      return invalid("the bounds must be finite with lo <= hi (dimension " + std::to_string(d) + ")");
    if (!std::isfinite(lr) || !(lr > 0.0)) return invalid("the step sizes must be finite and > 0 (dimension " + std::to_string(d) + ")");
    box->lo[d] = lo, box->hi[d] = hi, box->lr[d] = lr;
  }
  return AGP_OK;
}

static agp_status acq_moments(agp_ctx* ctx, const agp_acq_desc* d, int64_t n, const double* mu, const double* var, double* alpha,
                              double* dmu, double* dvar) {
  const char* who = "agp_acq_moments: ";
  agp::AcqParams p;
  AGPCHK(acq_check_desc(ctx, who, d, &p));
  if (n < 0 || (n > 0 && (!mu || !var || !alpha))) {
    ctx->err = std::string(who) + "n >= 0; mu, var and alpha_out must not be NULL";
    return AGP_ERR_INVALID;
  }
  if (n == 0) return AGP_OK;
  hipLaunchKernelGGL(agp::k_acq_moments, grid1(n), dim3(256), 0, ctx->stream, p, n, mu, var, alpha, dmu, dvar);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// k_acq_contract of nc <= 4096 particles; returns the number of column groups (what k_acq_step / k_acq_finish add up)
template <bool GRAD>
static int acq_contract_launch(hipStream_t s, const double* xs, int64_t ldx, int64_t nc, const double* Z, int64_t m, int64_t D,
                               const double* scales, int kind, double variance, const double* a, const double* W, int64_t ldw,
                               double* part, double* sc) {
  const int dpt = D <= 4 ? 1 : (D <= 16 ? 4 : (D <= 32 ? 8 : 16));
  const int64_t tpg = agp::pg_tiles_per_group(m, dpt), ntile = (m + agp::pg_ct(dpt) - 1) / agp::pg_ct(dpt), ng = (ntile + tpg - 1) / tpg;
  const dim3 grid((unsigned)((nc + agp::PG_RT - 1) / agp::PG_RT), (unsigned)ng), blk(agp::PG_THREADS);
#define AGP_ACQ_LAUNCH(DPT) \
  hipLaunchKernelGGL((agp::k_acq_contract<DPT, GRAD>), grid, blk, 0, s, xs, ldx, nc, Z, D, m, (int)D, scales, kind, variance, a, W, ldw, tpg, part, sc)
  if (dpt == 1) AGP_ACQ_LAUNCH(1);
  else if (dpt == 4) AGP_ACQ_LAUNCH(4);
  else if (dpt == 8) AGP_ACQ_LAUNCH(8);
  else AGP_ACQ_LAUNCH(16);
#undef AGP_ACQ_LAUNCH
  return (int)ng;
}

// What the ascent keeps on the handle: the groups' scalar sums of one chunk, the ADAM moments of one chunk, and the iterate and alpha
// of every particle of the call (grown by the call that has more starts than any before: the one place that may wait for the device)
struct AcqState {
  double *sc = nullptr, *mo = nullptr, *vo = nullptr;  // [2][PG_MAXGROUPS][4096] ; [4096][D] each
  double *X = nullptr, *A = nullptr;                  // [cap][D], [cap]
  int64_t cap = 0;
  agp_status ensure_chunk(agp_ctx* ctx, int64_t D, bool ascent) {
    if (!sc) AGPCHK(dmalloc(ctx, &sc, 2 * (int64_t)agp::PG_MAXGROUPS * agp::PG_CH));
    if (ascent && !mo) AGPCHK(dmalloc(ctx, &mo, (int64_t)agp::PG_CH * D));
    if (ascent && !vo) AGPCHK(dmalloc(ctx, &vo, (int64_t)agp::PG_CH * D));
    return AGP_OK;
  }
  agp_status ensure_particles(agp_ctx* ctx, int64_t R, int64_t D) {
    if (R <= cap) return AGP_OK;
    for (double** q : {&X, &A})
      if (*q) (void)hipFree(*q), *q = nullptr;
    cap = 0;
    AGPCHK(dmalloc(ctx, &X, R * D));
    AGPCHK(dmalloc(ctx, &A, R));
    cap = R;
    return AGP_OK;
  }
  ~AcqState() {
    for (double* q : {sc, mo, vo, X, A})
      if (q) (void)hipFree(q);
  }
};

// The predictor one pass runs on: inducing inputs with their scaled copy and norms (Svgp::ensure_zsc), the two objects (a, A), the
// count m with mp = rup64(m) (the extent of the GEMM; padding up to mp holds zeros), and a K*m / W pair of 4096 rows.  A, Kstar and W
// share the leading dimension ld >= mp.  With pending points (U != NULL) A is A0 = [[A, 0], [0, 0]] and the rank-one terms of A' stand
// apart (agp_acq_batch.h): W = K*m A0^T - (K*m U^T) N^T through W0 and G.
struct AcqPred {
  const double *Z, *Zsc, *zn, *a, *A;
  int64_t m, mp, ld;
  double *Kstar, *W;
  const double *U = nullptr, *N = nullptr;  // [64][ld], [ld][64]
  double *W0 = nullptr, *G = nullptr;       // [4096][ld], [4096][64]
};

// The augmented predictor (Z', a', A') of the pending points and its workspaces, sized once for m + ACQB_MAXPEND points: nothing of
// the latent's is resized or written.  ld = rup64(m + 64) whatever the number of pending points, so that no row ever moves.
struct AcqBatchWs {
  double *Z = nullptr, *Zsc = nullptr, *zn = nullptr, *a = nullptr, *A = nullptr;  // [mc][D], [ld][Dp], [ld], [ld], [ld][ld] (A0)
  double *U = nullptr, *N = nullptr;                                               // [64][ld]: u_b ; [ld][64]: -u_b / c_b
  double *Kstar = nullptr, *W = nullptr, *W0 = nullptr, *G = nullptr;              // [4096][ld] x 3, [4096][64]
  double *kv = nullptr, *w0 = nullptr, *w = nullptr, *g = nullptr, *c = nullptr;   // [ld] x 3, [64], [1]: one bordering step
  int32_t* bad = nullptr;                                                          // the latch of k_acqb_pivot
  int64_t m = 0, mc = 0, ld = 0;
  agp_status ensure(agp_ctx* ctx, int64_t m_, int64_t D) {
    if (A) return AGP_OK;
    m = m_, mc = m_ + agp::ACQB_MAXPEND, ld = rup64(mc);
    auto need = [&](double** q, int64_t n) { return *q ? AGP_OK : dmalloc(ctx, q, n); };  // (a call after a failed one goes on)
    AGPCHK(need(&Z, mc * D));
    if (kmm_usable(D)) {
      AGPCHK(need(&Zsc, ld * kmm_dp(D)));
      AGPCHK(need(&zn, ld));
    }
    AGPCHK(need(&a, ld));
    AGPCHK(need(&U, (int64_t)agp::ACQB_MAXPEND * ld));
    AGPCHK(need(&N, ld * agp::ACQB_MAXPEND));
    AGPCHK(need(&Kstar, (int64_t)agp::PG_CH * ld));
    AGPCHK(need(&W, (int64_t)agp::PG_CH * ld));
    AGPCHK(need(&W0, (int64_t)agp::PG_CH * ld));
    AGPCHK(need(&G, (int64_t)agp::PG_CH * agp::ACQB_MAXPEND));
    AGPCHK(need(&kv, ld));
    AGPCHK(need(&w0, ld));
    AGPCHK(need(&w, ld));
    AGPCHK(need(&g, agp::ACQB_MAXPEND));
    AGPCHK(need(&c, 1));
    if (!bad) {
      AGPCHK(dmalloc(ctx, &bad, 1));
      HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int32_t), ctx->stream));
    }
    AGPCHK(need(&A, ld * ld));  // (last: A != NULL says that all of them stand)
    return AGP_OK;
  }
  // (Z', a', A0) = (Z, a, A) of the latent, the padding zero-filled, no rank-one term; A has the leading dimension lda
  agp_status reset(agp_ctx* ctx, int64_t D, const double* Zl, const double* al, const double* Al, int64_t lda) {
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(A, 0, sizeof(double) * ld * ld, s));
    HIPCHK(ctx, hipMemsetAsync(a, 0, sizeof(double) * ld, s));
    HIPCHK(ctx, hipMemsetAsync(U, 0, sizeof(double) * agp::ACQB_MAXPEND * ld, s));
    HIPCHK(ctx, hipMemsetAsync(N, 0, sizeof(double) * ld * agp::ACQB_MAXPEND, s));
    HIPCHK(ctx, hipMemcpyAsync(Z, Zl, sizeof(double) * m * D, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(a, al, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpy2DAsync(A, sizeof(double) * ld, Al, sizeof(double) * lda, sizeof(double) * m, m, hipMemcpyDeviceToDevice, s));
    return AGP_OK;
  }
  // the bordering step for the point that stands in row n of Z' (n = m + b, b the number of points before it)
  agp_status border(agp_ctx* ctx, int64_t n, int64_t D, const double* scales, int kind, double variance, double kdiag) {
    hipStream_t s = ctx->stream;
    const int b = (int)(n - m);
    hipLaunchKernelGGL(agp::k_acqb_kvec, grid1(n), dim3(256), 0, s, (const double*)Z, n, (int)D, scales, kind, variance, kv);
    hipLaunchKernelGGL(agp::k_acqb_matvec, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const double*)A, ld, n, n, (const double*)kv, w0);
    if (b > 0)
      hipLaunchKernelGGL(agp::k_acqb_matvec, dim3((unsigned)((b + 3) / 4)), dim3(256), 0, s, (const double*)U, ld, (int64_t)b, n,
                         (const double*)kv, g);
    hipLaunchKernelGGL(agp::k_acqb_wsum, grid1(n), dim3(256), 0, s, n, b, (const double*)w0, (const double*)N, (const double*)g, w);
    hipLaunchKernelGGL(agp::k_acqb_pivot, dim3(1), dim3(256), 0, s, n, (const double*)kv, (const double*)w, kdiag, c, bad);
    hipLaunchKernelGGL(agp::k_acqb_store, grid1(n + 1), dim3(256), 0, s, n, b, ld, (const double*)w, (const double*)c, U, N);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  // the scaled copy and norms of the first n rows of Z', padded to rup64(n) rows, as Svgp::ensure_zsc makes the latent's
  agp_status rescale(agp_ctx* ctx, int64_t n, int64_t D, const double* scales) {
    if (!Zsc) return AGP_OK;
    const int64_t np = rup64(n);
    hipLaunchKernelGGL((agp::k_scale_rows<double>), dim3((unsigned)((np + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)Z, D, n, np,
                       D, kmm_dp(D), scales, Zsc, zn);
    LAUNCHCHK(ctx);
    return AGP_OK;
  }
  AcqPred pred(int64_t n) const { return AcqPred{Z, Zsc, zn, a, A, n, rup64(n), ld, Kstar, W, U, N, W0, G}; }
  ~AcqBatchWs() {
    for (double* q : {Z, Zsc, zn, a, A, U, N, Kstar, W, W0, G, kv, w0, w, g, c})
      if (q) (void)hipFree(q);
    if (bad) (void)hipFree(bad);
  }
};

// What the passes read of the model: one latent's predictor as Svgp<T>::ensure_pred leaves it, with the chunk workspaces that the
// acquisition functions share with predict_f_grad.  Filled by the handle (SvgpBase::acq_open), where the pointer casts happen once.
struct AcqModel {
  agp_ctx* ctx;  // every launch goes to ctx->stream
  int64_t D, m, mp;
  int kind;         // the latent's kernel, ...
  double variance;  // ... its variance as the kernels take it (Svgp<T>::kvar), ...
  double kdiag;     // ... and k(x, x) + jitter
  const double* scales;
  AcqPred pred;  // the latent's own objects with the shared Kstar and W
  double* part;  // [2][PG_MAXGROUPS][4096][D]: the groups' partial gradients
};

// K*m of n <= 4096 rows of x (pitched by ldx) on the predictor pr, and W = K*m A': the two launches every pass begins with
static agp_status acq_kstar_w(const AcqModel& M, const AcqPred& pr, const double* x, int64_t ldx, int64_t n, double* Kstar, double* W) {
  (void)launch_kernelmatrix<double>(M.ctx, M.ctx->stream, x, ldx, (const int64_t*)nullptr, n, pr.Z, M.D, pr.m, M.D, M.scales, M.kind,
                                    M.variance, Kstar, pr.ld, rup64(n), pr.mp, 0, 0.0, (const double*)nullptr, (double*)nullptr, 0, 0,
                                    pr.Zsc, pr.zn);
  LAUNCHCHK(M.ctx);
  return gemm_nt<double, EPI_STORE>(M.ctx, Kstar, pr.ld, pr.A, pr.ld, rup64(n), pr.mp, pr.mp, 0, W, pr.ld, nullptr, 0, nullptr, nullptr,
                                    nullptr, 0);
}

// the arguments that the two calls with pending points share; noise is tau2
static agp_status acqb_check_pending(agp_ctx* ctx, const char* who, int64_t D, const void* xp, int64_t ldp, int64_t n, int64_t q,
                                     double noise) {
  auto invalid = [&](const char* what) {
    ctx->err = std::string(who) + what;
    return AGP_ERR_INVALID;
  };
  if (n < 0 || q < 1 || n > AGP_ACQ_MAX_PENDING || q > AGP_ACQ_MAX_PENDING || n + q > AGP_ACQ_MAX_PENDING)
    return invalid("n_pending >= 0, q >= 1 and n_pending + q <= AGP_ACQ_MAX_PENDING (64)");
  if (!std::isfinite(noise) || noise < 0.0) return invalid("noise must be finite and >= 0");
  if (n > 0 && !xp) return invalid("xp must be given when n_pending > 0");
  if (n > 0 && ldp < D) return invalid("ldp >= D");
  return AGP_OK;
}

// x0, the options, then the starts and outputs of a maximiser (acq_check_max_out), in the order the three maximisers refuse in
static agp_status acq_check_ascent(agp_ctx* ctx, const char* who, int64_t D, const void* x0, int64_t ldx0, int64_t R, int64_t per,
                                   const agp_pw_ascent_opts* o, agp::PwAscentBox* box, const char* xname, const char* ldname,
                                   bool x_required, const void* x_out, int64_t ldxo, bool other_out, const void* best_x, int64_t ldb) {
  if (!x0) {
    ctx->err = std::string(who) + "x0 must be given";
    return AGP_ERR_INVALID;
  }
  AGPCHK(acq_check_opts(ctx, who, D, o, box));
  return acq_check_max_out(ctx->err, who, D, R, per, ldx0, xname, ldname, x_required, x_out, ldxo, other_out, best_x, ldb);
}

// The host driver of the acquisition functions of one handle: the state the calls keep and the four entry points that are not
// joint (AcqJointDriver, agp_acq_joint_host.h, builds on this one).  Per chunk of 4096 points and pass: K*m and W (acq_kstar_w),
// k_acq_contract, and one finishing kernel (k_acq_finish, or k_acq_step with the ADAM update): four launches, nothing waits for the
// stream.  The pending points condition the variance through the augmented predictor (Z', a', A') of AcqBatchWs, built by bordering
// in the order of the points and kept as A0 and its rank-one terms; the passes then run on it with m' = m + n.  With no pending
// point the latent's own objects are passed, so those calls are the launches of evaluate / maximize.
// Every entry point refuses in one order -- the handle's acq_check, the family's own arguments, x0, the options, the outputs and
// leading dimensions, then the return of an empty call -- and only then opens the handle, which is the first thing that allocates.
struct AcqDriver {
  AcqState acq;
  AcqBatchWs acqb;

  // K*m, W and the contraction of nc <= 4096 points (rows of xs pitched by ldx) into M.part / acq.sc: three launches, on the
  // predictor pr (the latent's own objects, or the augmented ones of the pending points)
  template <bool GRAD>
  agp_status pass(const AcqModel& M, const AcqPred& pr, const double* xs, int64_t ldx, int64_t nc, int* ng) {
    AGPCHK(acq_kstar_w(M, pr, xs, ldx, nc, pr.Kstar, pr.U ? pr.W0 : pr.W));
    if (pr.U) {  // the rank-one terms of the pending points: G = K*m' U^T, W = W0 - G N^T
      AGPCHK((gemm_nt<double, EPI_STORE>(M.ctx, pr.Kstar, pr.ld, pr.U, pr.ld, rup64(nc), agp::ACQB_MAXPEND, pr.mp, 0, pr.G,
                                         agp::ACQB_MAXPEND, nullptr, 0, nullptr, nullptr, nullptr, 0)));
      AGPCHK((gemm_nt<double, EPI_EMINUS>(M.ctx, pr.G, agp::ACQB_MAXPEND, pr.N, agp::ACQB_MAXPEND, rup64(nc), pr.mp, agp::ACQB_MAXPEND, 0,
                                          pr.W, pr.ld, pr.W0, pr.ld, nullptr, nullptr, nullptr, 0)));
    }
    *ng = acq_contract_launch<GRAD>(M.ctx->stream, xs, ldx, nc, pr.Z, pr.m, M.D, M.scales, M.kind, M.variance, pr.a, (const double*)pr.W,
                                    pr.ld, M.part, acq.sc);
    LAUNCHCHK(M.ctx);
    return AGP_OK;
  }
  // alpha (and grad, nullable) at nt points in chunks of 4096: four launches per chunk
  agp_status eval(const AcqModel& M, const AcqPred& pr, const agp::AcqParams& p, const double* xt, int64_t ldx, int64_t nt,
                  double* alpha_out, double* grad_out, int64_t ldg) {
    for (int64_t s = 0; s < nt; s += agp::PG_CH) {
      const int64_t nc = (nt - s) < agp::PG_CH ? (nt - s) : agp::PG_CH;
      const double* xs = xt + s * ldx;
      int ng = 0;
      if (grad_out) AGPCHK(pass<true>(M, pr, xs, ldx, nc, &ng));
      else AGPCHK(pass<false>(M, pr, xs, ldx, nc, &ng));
      hipLaunchKernelGGL(agp::k_acq_finish, grid1(nc * (grad_out ? M.D : 1)), dim3(256), 0, M.ctx->stream, p, nc, (int)M.D, ng,
                         (const double*)(grad_out ? M.part : nullptr), (const double*)acq.sc, M.scales, M.kdiag, alpha_out + s,
                         grad_out ? grad_out + s * ldg : (double*)nullptr, ldg);
      LAUNCHCHK(M.ctx);
    }
    return AGP_OK;
  }
  // The ADAM ascent of R starts of q particles each into acq.X / acq.A: chunk after chunk of floor(4096 / q) starts (a start never
  // straddles two chunks), each through all T steps and one more pass, which leaves alpha at the last x.  The two things that differ
  // between the ascents are passed in:
  //   pass(x, s, ns, fin, &ng)            the pass of the chunk's ns starts, the first of which is start s; without gradient when fin
  //   step(x, s, ns, ng, fin, c1, c2)     the launch that ends the pass: the ADAM update with the bias corrections c1, c2, or at fin
  //                                       whatever closes the ascent
  template <class Pass, class Step>
  agp_status ascend(const AcqModel& M, const agp::PwAscentBox& box, const agp_pw_ascent_opts* o, const double* x0, int64_t ldx0,
                    int64_t R, int64_t q, Pass pass, Step step) {
#pragma clang fp contract(off)
    const int64_t spc = agp::PG_CH / q;
    for (int64_t s = 0; s < R; s += spc) {
      const int64_t ns = (R - s) < spc ? (R - s) : spc, np = ns * q;
      double* x = acq.X + s * q * M.D;
      hipLaunchKernelGGL(agp::k_acq_init, grid1(np * M.D), dim3(256), 0, M.ctx->stream, np, (int)M.D, x0 + s * q * ldx0, ldx0, box, x,
                         acq.mo, acq.vo);
      LAUNCHCHK(M.ctx);
      double b1k = 1.0, b2k = 1.0;
      for (int k = 0; k <= o->steps; ++k) {
        const bool fin = k == o->steps;  // the pass after the last step: alpha at the final x
        int ng = 0;
        AGPCHK(pass(x, s, ns, fin, &ng));
        if (!fin) b1k *= o->beta1, b2k *= o->beta2;
        AGPCHK(step(x, s, ns, ng, fin, 1.0 - b1k, 1.0 - b2k));
      }
    }
    return AGP_OK;
  }
  // the ascent of single points on the predictor pr
  agp_status ascend_points(const AcqModel& M, const AcqPred& pr, const agp::AcqParams& p, const agp::PwAscentBox& box,
                           const agp_pw_ascent_opts* o, const double* x0, int64_t ldx0, int64_t R) {
    return ascend(
        M, box, o, x0, ldx0, R, 1,
        [&](double* x, int64_t, int64_t nc, bool fin, int* ng) {
          return fin ? pass<false>(M, pr, x, M.D, nc, ng) : pass<true>(M, pr, x, M.D, nc, ng);
        },
        [&](double* x, int64_t s, int64_t nc, int ng, bool fin, double c1, double c2) -> agp_status {
          hipLaunchKernelGGL(agp::k_acq_step, grid1(nc * (fin ? 1 : M.D)), dim3(256), 0, M.ctx->stream, p, nc, (int)M.D, ng,
                             (const double*)M.part, (const double*)acq.sc, M.scales, M.kdiag, o->beta1, o->beta2, c1, c2, o->eps, box,
                             (int)fin, x, acq.mo, acq.vo, acq.A + s);
          LAUNCHCHK(M.ctx);
          return AGP_OK;
        });
  }
  // what a maximiser hands back of every start: the iterates (R rows of D values each) and alpha, both nullable
  agp_status copy_out(const AcqModel& M, int64_t rows, int64_t R, double* x_out, int64_t ldxo, double* a_out) {
    if (x_out)
      HIPCHK(M.ctx, hipMemcpy2DAsync(x_out, sizeof(double) * ldxo, acq.X, sizeof(double) * M.D, sizeof(double) * M.D, rows,
                                     hipMemcpyDeviceToDevice, M.ctx->stream));
    if (a_out) HIPCHK(M.ctx, hipMemcpyAsync(a_out, acq.A, sizeof(double) * R, hipMemcpyDeviceToDevice, M.ctx->stream));
    return AGP_OK;
  }
  // (Z', a', A') of the latent with the n pending points of xp bordered on, in their order
  agp_status begin(const AcqModel& M, const double* xp, int64_t ldp, int64_t n, double noise) {
    AGPCHK(acqb.reset(M.ctx, M.D, M.pred.Z, M.pred.a, M.pred.A, M.mp));
    if (n == 0) return AGP_OK;
    HIPCHK(M.ctx, hipMemcpy2DAsync(acqb.Z + M.m * M.D, sizeof(double) * M.D, xp, sizeof(double) * ldp, sizeof(double) * M.D, n,
                                   hipMemcpyDeviceToDevice, M.ctx->stream));
    for (int64_t i = 0; i < n; ++i) AGPCHK(border(M, M.m + i, noise));
    return acqb.rescale(M.ctx, M.m + n, M.D, M.scales);
  }
  agp_status border(const AcqModel& M, int64_t n, double noise) {
#pragma clang fp contract(off)
    return acqb.border(M.ctx, n, M.D, M.scales, M.kind, M.variance, M.kdiag + noise);
  }

  static agp_status evaluate(SvgpBase& h, int l, const agp_acq_desc* d, const double* xt, int64_t ldx, int64_t nt, double* alpha_out,
                             double* grad_out, int64_t ldg) {
    const char* who = "agp_svgp_acquisition: ";
    agp::AcqParams p;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acq_check_eval_out(h.ctx->err, who, "n_t", "xt", h.desc.D, nt, xt, ldx, alpha_out, grad_out, ldg));
    if (nt == 0) return AGP_OK;
    AcqModel M;
    AcqDriver* dr;
    AGPCHK(h.acq_open(l, false, &M, &dr, nullptr));
    return dr->eval(M, M.pred, p, xt, ldx, nt, alpha_out, grad_out, ldg);
  }
  static agp_status maximize(SvgpBase& h, int l, const agp_acq_desc* d, const double* x0, int64_t ldx0, int64_t R,
                             const agp_pw_ascent_opts* o, double* x_out, int64_t ldxo, double* a_out, double* best_x, double* best_a,
                             int64_t* best_idx) {
    const char* who = "agp_svgp_acq_maximize: ";
    const int64_t D = h.desc.D;
    agp::AcqParams p;
    agp::PwAscentBox box;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acq_check_ascent(h.ctx, who, D, x0, ldx0, R, 1, o, &box, "x_out", "ldxo", false, x_out, ldxo,
                            a_out || best_x || best_a || best_idx, nullptr, 0));
    AcqModel M;
    AcqDriver* dr;
    AGPCHK(h.acq_open(l, true, &M, &dr, nullptr));
    AGPCHK(dr->acq.ensure_particles(M.ctx, R, D));
    AGPCHK(dr->ascend_points(M, M.pred, p, box, o, x0, ldx0, R));
    if (best_x || best_a || best_idx) {
      hipLaunchKernelGGL(agp::k_pw_ascent_best, dim3(1), dim3(256), 0, M.ctx->stream, (const double*)dr->acq.X, (const double*)dr->acq.A,
                         R, D, 1.0, best_x, D, best_a, best_idx);
      LAUNCHCHK(M.ctx);
    }
    return dr->copy_out(M, R, R, x_out, ldxo, a_out);
  }
  static agp_status evaluate_pending(SvgpBase& h, int l, const agp_acq_desc* d, const double* xp, int64_t ldp, int64_t n, double noise,
                                     const double* xt, int64_t ldx, int64_t nt, double* alpha_out, double* grad_out, int64_t ldg) {
    const char* who = "agp_svgp_acquisition_pending: ";
    agp::AcqParams p;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acqb_check_pending(h.ctx, who, h.desc.D, xp, ldp, n, 1, noise));
    AGPCHK(acq_check_eval_out(h.ctx->err, who, "n_t", "xt", h.desc.D, nt, xt, ldx, alpha_out, grad_out, ldg));
    if (nt == 0) return AGP_OK;
    AcqModel M;
    AcqDriver* dr;
    AGPCHK(h.acq_open(l, false, &M, &dr, nullptr));
    if (n == 0) return dr->eval(M, M.pred, p, xt, ldx, nt, alpha_out, grad_out, ldg);
    AGPCHK(dr->acqb.ensure(M.ctx, M.m, M.D));
    AGPCHK(dr->begin(M, xp, ldp, n, noise));
    return dr->eval(M, dr->acqb.pred(M.m + n), p, xt, ldx, nt, alpha_out, grad_out, ldg);
  }
  static agp_status maximize_batch(SvgpBase& h, int l, const agp_acq_desc* d, const double* xp, int64_t ldp, int64_t n, double noise,
                                   int64_t q, const double* x0, int64_t ldx0, int64_t R, const agp_pw_ascent_opts* o, double* xb_out,
                                   int64_t ldxb, double* ab_out, int64_t* idxb_out) {
    const char* who = "agp_svgp_acq_maximize_batch: ";
    const int64_t D = h.desc.D;
    agp::AcqParams p;
    agp::PwAscentBox box;
    AGPCHK(h.acq_check(who, l, d, &p));
    AGPCHK(acqb_check_pending(h.ctx, who, D, xp, ldp, n, q, noise));
    AGPCHK(acq_check_ascent(h.ctx, who, D, x0, ldx0, R, 1, o, &box, "xb_out", "ldxb", true, xb_out, ldxb, false, nullptr, 0));
    AcqModel M;
    AcqDriver* dr;
    AGPCHK(h.acq_open(l, true, &M, &dr, nullptr));
    AcqBatchWs& b = dr->acqb;
    AGPCHK(dr->acq.ensure_particles(M.ctx, R, D));
    AGPCHK(b.ensure(M.ctx, M.m, D));
    if (n > 0 || q > 1) AGPCHK(dr->begin(M, xp, ldp, n, noise));
    for (int64_t i = 0; i < q; ++i) {
      const int64_t np = n + i;  // the points the round is conditioned on: the caller's and the winners before
      AGPCHK(dr->ascend_points(M, np == 0 ? M.pred : b.pred(M.m + np), p, box, o, x0, ldx0, R));
      double* win = b.Z + (M.m + np) * D;  // the winner goes device to device into the next row of the pending list
      hipLaunchKernelGGL(agp::k_pw_ascent_best, dim3(1), dim3(256), 0, M.ctx->stream, (const double*)dr->acq.X, (const double*)dr->acq.A,
                         R, D, 1.0, win, D, ab_out ? ab_out + i : (double*)nullptr, idxb_out ? idxb_out + i : (int64_t*)nullptr);
      LAUNCHCHK(M.ctx);
      HIPCHK(M.ctx, hipMemcpyAsync(xb_out + i * ldxb, win, sizeof(double) * D, hipMemcpyDeviceToDevice, M.ctx->stream));
      if (i + 1 < q) {
        AGPCHK(dr->border(M, M.m + np, noise));
        AGPCHK(b.rescale(M.ctx, M.m + np + 1, D, M.scales));
      }
    }
    return AGP_OK;
  }
};
