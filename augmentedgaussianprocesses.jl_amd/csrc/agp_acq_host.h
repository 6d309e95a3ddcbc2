// agp_acq_host.h -- host driver of the acquisition functions (kernels: agp_acq.h; include/agp_hip.h "ACQUISITION FUNCTIONS"): the
// argument checks of agp_acq_desc and agp_pw_ascent_opts, which touch nothing, agp_acq_moments, the launch of k_acq_contract and the
// particle state of the ascent.  Svgp<T>::acquisition / acq_maximize (agp_capi.hip) drive them with the predictor's workspaces.
// Batch acquisition (kernels: agp_acq_batch.h): AcqPred names the predictor a pass runs on -- the latent's own objects, or the
// augmented ones of AcqBatchWs, which the bordering launches below extend by one pending point at a time.
#pragma once
#include <cmath>
#include <string>

#include "agp_acq.h"
#include "agp_acq_batch.h"
#include "agp_blas_host.h"  // kmm_usable, kmm_dp
#include "agp_ctx.h"

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
