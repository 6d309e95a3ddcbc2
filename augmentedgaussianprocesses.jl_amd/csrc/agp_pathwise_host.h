// agp_pathwise_host.h -- host driver of pathwise posterior sampling (kernels: agp_pathwise.h): struct agp_pathwise, the draw that
// the C ABI hands out and that owns everything it evaluates with, the scratch of its construction (PwScratch) and the pw_*
// routines: argument checks, spectral tables, per-latent snapshot, features, the inverse factor, the chunked evaluation (pw_eval) and
// the chunked input gradients (pw_eval_grad) and the multi-start ascent (pw_maximize).  The
// models build draws in Svgp<T>::pathwise_draw (agp_capi.hip) and its overrides; the agp_pathwise_* entry points are in agp_capi.hip.
#pragma once
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "agp_blas_host.h"
#include "agp_chol_host.h"
#include "agp_ctx.h"
#include "agp_hyper.h"  // k_gemm_tn
#include "agp_pathwise.h"
#include "agp_rand.h"
#include "agp_svgp_base.h"

// ---- pathwise sampling (include/agp_hip.h, "PATHWISE SAMPLING"; device code in agp_pathwise.h) -------------------------------------
// A draw owns everything it evaluates with: per latent the snapshot of the kernel (kind, variance, scales), of Z with its ready-made
// kernel-matrix tiles, the spectral tables, [W' | V'] (Sp x (Lp + mp), sample-major: the B side of the evaluation's one gemm_nt) and
// E; shared by the latents the workspace [Phi(x) | k(x, Z)] of one chunk of test points and the chunk's result before it is copied
// into the caller's rows.
struct agp_pathwise {
  agp_ctx* ctx = nullptr;
  int nl = 0, L = 0, S = 0;
  int64_t Lp = 0, Sp = 0, m = 0, mp = 0, D = 0, ldw = 0, CH = 0;
  struct Lat {
    int kind = AGP_K_SQEXP;
    double variance = 1.0, amp = 0.0;
    double *scales = nullptr, *Z = nullptr, *Zsc = nullptr, *zn = nullptr, *omega = nullptr, *phase = nullptr, *WV = nullptr,
           *E = nullptr;
  };
  std::vector<Lat> lat;
  double *ws = nullptr, *Fs = nullptr;
  // the gradient's own buffers, allocated by its first call (pw_grad_buffers): the per-dimension operand Wd, the same size as ws,
  // and the slabs of GD dimensions before they are transposed into the caller's rows
  double *ws2 = nullptr, *Gs = nullptr;
  int GD = 0;
  // the ascent's particle state (pw_maximize): the final x (mx_cap x D) and f (mx_cap) of every particle, grown by the call that needs more
  double *mxX = nullptr, *mxF = nullptr;
  int64_t mx_cap = 0;
  ~agp_pathwise() {
    for (auto& a : lat)
      for (double* q : {a.scales, a.Z, a.Zsc, a.zn, a.omega, a.phase, a.WV, a.E})
        if (q) (void)hipFree(q);
    for (double* q : {ws, Fs, ws2, Gs, mxX, mxF})
      if (q) (void)hipFree(q);
  }
};
// device buffers that live as long as one call
struct PwScratch {
  std::vector<void*> v;
  ~PwScratch() {
    for (void* q : v) (void)hipFree(q);
  }
  template <typename U>
  agp_status get(agp_ctx* c, U** q, int64_t n) {
    AGPCHK(dmalloc(c, q, n));
    v.push_back(*q);
    return AGP_OK;
  }
};
constexpr int64_t PW_MAX = 65536, PW_CTR_MAX = (int64_t)0xFFFFFFFFll;
static agp_status pw_check_spectral(agp_ctx* ctx, const char* who, int64_t D, int64_t L, int64_t t) {
  if (L < 1 || L > PW_MAX) {
    ctx->err = std::string(who) + ": n_features must lie in [1, 65536] (got " + std::to_string(L) + ")";
    return AGP_ERR_INVALID;
  }
  if (D < 1 || L * D > PW_CTR_MAX) {
    ctx->err = std::string(who) + ": D >= 1 and n_features * D below 2^32 (one 32-bit counter word per frequency element)";
    return AGP_ERR_INVALID;
  }
  if (t < 0 || t > PW_CTR_MAX) {
    ctx->err = std::string(who) + ": the draw counter t is one 32-bit word of the generator's counter, 0 <= t < 2^32";
    return AGP_ERR_INVALID;
  }
  return AGP_OK;
}
static agp_status pw_check_draw(agp_ctx* ctx, int64_t m, int64_t D, int64_t L, int64_t S, int64_t t, agp_pathwise** out) {
  const char* who = "agp_svgp_pathwise_draw";
  if (!out) {
    ctx->err = std::string(who) + ": out must be given";
    return AGP_ERR_INVALID;
  }
  AGPCHK(pw_check_spectral(ctx, who, D, L, t));
  if (S < 1 || S > PW_MAX) {
    ctx->err = std::string(who) + ": n_samples must lie in [1, 65536] (got " + std::to_string(S) + ")";
    return AGP_ERR_INVALID;
  }
  if (L * S > PW_CTR_MAX || m * S > PW_CTR_MAX) {
    ctx->err = std::string(who) + ": n_features * n_samples and m * n_samples must stay below 2^32 (counter words of W and E)";
    return AGP_ERR_INVALID;
  }
  return AGP_OK;
}
static agp_status pw_spectral(agp_ctx* ctx, int kind, int64_t D, int64_t L, uint64_t seed, int64_t t, int latent, double* omega,
                              double* phase) {
  hipLaunchKernelGGL(agp::k_pw_spectral, grid1(L * D), dim3(256), 0, ctx->stream, L * D, D, kind, seed, (uint32_t)t,
                     (uint32_t)(4 + 8 * latent), omega, phase);
  LAUNCHCHK(ctx);
  return AGP_OK;
}
// the empty draw: sizes, the chunk of the evaluation workspace under AGP_PATHWISE_WS_BYTES, the shared buffers
static agp_status pw_create(agp_ctx* ctx, int nl, int64_t m, int64_t D, int L, int S, std::unique_ptr<agp_pathwise>* out) {
  std::unique_ptr<agp_pathwise> p(new agp_pathwise());
  p->ctx = ctx, p->nl = nl, p->L = L, p->S = S, p->m = m, p->D = D;
  p->Lp = rup64(L), p->Sp = rup64(S), p->mp = rup64(m), p->ldw = p->Lp + p->mp;
  const int64_t per_point = 8 * (p->ldw + p->Sp);
  p->CH = std::min<int64_t>(4096, std::max<int64_t>(64, (int64_t)AGP_PATHWISE_WS_BYTES / per_point / 64 * 64));
  p->lat.resize(nl);
  AGPCHK(dmalloc(ctx, &p->ws, p->CH * p->ldw));
  AGPCHK(dmalloc(ctx, &p->Fs, p->Sp * p->CH));
  *out = std::move(p);
  return AGP_OK;
}
// one latent's snapshot and tables: kernel, scales (D + 1 doubles as the handle keeps them: the variance behind the scales), Z
// (m x D, dense), its kernel-matrix tiles, Omega and the phases, W (into the left columns of [W' | V']) and E (mp x Sp)
static agp_status pw_add_latent(agp_pathwise& p, int l, int kind, double variance, const double* scales_dev, const double* Z_dev,
                                uint64_t seed, int64_t t) {
  agp_ctx* ctx = p.ctx;
  agp_pathwise::Lat& a = p.lat[l];
  a.kind = kind, a.variance = variance, a.amp = std::sqrt(2.0 * variance / (double)p.L);
  AGPCHK(dmalloc(ctx, &a.scales, p.D + 1));
  AGPCHK(dmalloc(ctx, &a.Z, p.m * p.D));
  AGPCHK(dmalloc(ctx, &a.omega, (int64_t)p.L * p.D));
  AGPCHK(dmalloc(ctx, &a.phase, p.L));
  AGPCHK(dmalloc(ctx, &a.WV, p.Sp * p.ldw));
  AGPCHK(dmalloc(ctx, &a.E, p.mp * p.Sp));
  HIPCHK(ctx, hipMemcpyAsync(a.scales, scales_dev, sizeof(double) * (p.D + 1), hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(a.Z, Z_dev, sizeof(double) * p.m * p.D, hipMemcpyDeviceToDevice, ctx->stream));
  if (kmm_usable(p.D)) {
    const int Dp = kmm_dp(p.D);
    AGPCHK(dmalloc(ctx, &a.Zsc, p.mp * Dp));
    AGPCHK(dmalloc(ctx, &a.zn, p.mp));
    hipLaunchKernelGGL((agp::k_scale_rows<double>), dim3((unsigned)((p.mp + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)a.Z,
                       p.D, p.m, p.mp, p.D, Dp, (const double*)a.scales, a.Zsc, a.zn);
    LAUNCHCHK(ctx);
  }
  AGPCHK(pw_spectral(ctx, kind, p.D, p.L, seed, t, l, a.omega, a.phase));
  const uint32_t s0 = (uint32_t)(4 + 8 * l);
  HIPCHK(ctx, hipMemsetAsync(a.WV, 0, sizeof(double) * p.Sp * p.ldw, ctx->stream));
  hipLaunchKernelGGL(agp::k_pw_table, grid1(p.Lp * p.Sp), dim3(256), 0, ctx->stream, (int64_t)p.L, (int64_t)p.S, p.Lp, p.Sp,
                     (int64_t)1, p.ldw, 0, seed, (uint32_t)t, s0 + agp::PW_STREAM_W, a.WV);
  hipLaunchKernelGGL(agp::k_pw_table, grid1(p.mp * p.Sp), dim3(256), 0, ctx->stream, p.m, (int64_t)p.S, p.mp, p.Sp, p.Sp,
                     (int64_t)1, 1, seed, (uint32_t)t, s0 + agp::PW_STREAM_E, a.E);
  LAUNCHCHK(ctx);
  return AGP_OK;
}
// Phi(x) of n points (rows 0 .. rup64(n) of the workspace, left Lp columns; padding rows and columns exact zeros); SIN: the
// features' derivative -amp sin(.) instead (the gradient's A block)
template <bool SIN = false>
static agp_status pw_features(agp_pathwise& p, const agp_pathwise::Lat& a, const double* x, int64_t ldx, int64_t n) {
  hipLaunchKernelGGL(agp::k_pw_features<SIN>, dim3((unsigned)(p.Lp / TILE), (unsigned)(rup64(n) / TILE)), dim3(256), 0, p.ctx->stream, x,
                     ldx, n, p.D, (const double*)a.scales, (const double*)a.omega, (const double*)a.phase, (int64_t)p.L, a.amp, p.ws,
                     p.ldw);
  LAUNCHCHK(p.ctx);
  return AGP_OK;
}
// PW (mp x Sp) = Phi(Z) W, the rows of Z in chunks of the evaluation workspace
static agp_status pw_phi_W(agp_pathwise& p, int l, double* PW) {
  const agp_pathwise::Lat& a = p.lat[l];
  HIPCHK(p.ctx, hipMemsetAsync(PW, 0, sizeof(double) * p.mp * p.Sp, p.ctx->stream));
  for (int64_t r0 = 0; r0 < p.m; r0 += p.CH) {
    const int64_t nc = std::min<int64_t>(p.CH, p.m - r0), nq = rup64(nc);
    AGPCHK(pw_features(p, a, a.Z + r0 * p.D, p.D, nc));
    AGPCHK((gemm_nt<double, EPI_STORE>(p.ctx, p.ws, p.ldw, a.WV, p.ldw, nq, p.Sp, p.Lp, 0, PW + r0 * p.Sp, p.Sp, nullptr, 0, nullptr,
                                       nullptr, nullptr, 0)));
  }
  return AGP_OK;
}
// X = chol_lower(A)^-1 of a padded SPD matrix (A is destroyed), strict upper triangle zero: the driver of agp_spd_inverse
static agp_status pw_inverse_factor(agp_ctx* ctx, PwScratch& sc, double* A, const double* A_src, int64_t lds, int64_t n, int64_t np,
                                    double scale, double* X) {
  double* Dg = nullptr;
  int32_t* info = nullptr;
  AGPCHK(sc.get(ctx, &Dg, np * TILE));
  AGPCHK(sc.get(ctx, &info, 1));
  auto fill = [&]() {
    hipLaunchKernelGGL((agp::k_copy2d<double>), grid2(np, np), blk2, 0, ctx->stream, A_src, lds, n, n, A, np, np, np, 1.0, scale);
  };
  fill();
  HIPCHK(ctx, hipMemsetAsync(X, 0, sizeof(double) * np * np, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
  PotrfReq<double> rq{};
  rq.A = A, rq.ld = np, rq.n = np, rq.X = X, rq.ldx = np, rq.Dg = Dg, rq.do_x = 1, rq.info_dev = info, rq.nvalid = n;
  AGPCHK(potrf_fused<double>(ctx, rq));
  if (chol_use_dag(ctx, np / TILE)) {
    bool lost = false;
    AGPCHK(dag_lost_dependency(ctx, info, &lost));
    if (lost) {
      fill();
      AGPCHK(potrf_fused<double>(ctx, rq));
    }
  }
  hipLaunchKernelGGL((agp::k_zero_strict_upper<double>), grid2(np, np), blk2, 0, ctx->stream, X, np, np);
  LAUNCHCHK(ctx);
  int32_t hinfo = 0;
  HIPCHK(ctx, hipMemcpyAsync(&hinfo, info, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (hinfo != 0) {
    ctx->err = "agp_svgp_pathwise_draw: -2 eta2 is not positive definite; leading minor " + std::to_string(hinfo);
    return AGP_ERR_NOT_POSDEF;
  }
  return AGP_OK;
}
// C (M x N, ldc) = A (K x M)' B (K x N), all multiples of 64
static agp_status pw_gemm_tn(agp_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t M, int64_t N, int64_t K,
                             double* Cm, int64_t ldc) {
  hipLaunchKernelGGL((agp::k_gemm_tn<double, 1>), dim3((unsigned)(N / TILE), (unsigned)(M / TILE)), dim3(NTHREADS), 0, ctx->stream, A, lda,
                     B, ldb, K, Cm, ldc);
  LAUNCHCHK(ctx);
  return AGP_OK;
}
// the paths of latent l at one chunk of nc <= CH points, into out[s][0 .. nc) (rows pitched by ldo)
static agp_status pw_eval_chunk(agp_pathwise& p, int l, const double* xs, int64_t ldx, int64_t nc, double* out, int64_t ldo) {
  agp_ctx* ctx = p.ctx;
  const agp_pathwise::Lat& a = p.lat[l];
  const int64_t nq = rup64(nc);
  AGPCHK(pw_features(p, a, xs, ldx, nc));
  const int rc = launch_kernelmatrix<double>(ctx, ctx->stream, xs, ldx, (const int64_t*)nullptr, nc, (const double*)a.Z, p.D, p.m,
                                             p.D, (const double*)a.scales, a.kind, a.variance, p.ws + p.Lp, p.ldw, nq, p.mp, 0,
                                             0.0, (const double*)nullptr, (double*)nullptr, (int64_t)0, 0, (const double*)a.Zsc,
                                             (const double*)a.zn);
  LAUNCHCHK(ctx);
  if (rc < 0) return AGP_ERR_NOMEM;
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, a.WV, p.ldw, p.ws, p.ldw, p.Sp, nq, p.ldw, 0, p.Fs, p.CH, nullptr, 0, nullptr, nullptr,
                                     nullptr, 0)));
  HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(double) * ldo, p.Fs, sizeof(double) * p.CH, sizeof(double) * nc, p.S,
                               hipMemcpyDeviceToDevice, ctx->stream));
  return AGP_OK;
}
static agp_status pw_eval(agp_pathwise& p, const double* xt, int64_t ldx, int64_t nt, double* out, int64_t ldo) {
  for (int l = 0; l < p.nl; ++l)
    for (int64_t s = 0; s < nt; s += p.CH)
      AGPCHK(pw_eval_chunk(p, l, xt + s * ldx, ldx, std::min<int64_t>(p.CH, nt - s), out + ((int64_t)l * p.S) * ldo + s, ldo));
  return AGP_OK;
}
// The gradient's buffers, on its first call: Wd (CH x ldw) and the slabs of GD dimensions (GD x Sp x CH).  GD = min(D, PW_GD), fewer
// where the slabs would exceed AGP_PATHWISE_WS_BYTES (a function of the draw's sizes alone).
static agp_status pw_grad_buffers(agp_pathwise& p) {
  if (p.ws2 && p.Gs) return AGP_OK;
  const int64_t slab = 8 * p.Sp * p.CH;
  const int gd = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.D, agp::PW_GD), (int64_t)AGP_PATHWISE_WS_BYTES / slab));
  if (!p.ws2) AGPCHK(dmalloc(p.ctx, &p.ws2, p.CH * p.ldw));
  if (!p.Gs) AGPCHK(dmalloc(p.ctx, &p.Gs, (int64_t)gd * p.Sp * p.CH));
  p.GD = gd;
  return AGP_OK;
}
// d f_s / d x (include/agp_hip.h, agp_pathwise_eval_grad; kernels and the formulation: agp_pathwise.h).  Per chunk and latent: the
// values, if asked for, by pw_eval_chunk; the base workspace [A | C] into ws; then per dimension the operand into ws2, the
// evaluation's gemm_nt against [W' | V'] into one slab, and after every GD dimensions the transposing scatter into g[s][i][d].
static agp_status pw_eval_grad(agp_pathwise& p, const double* xt, int64_t ldx, int64_t nt, double* f_out, int64_t ldo, double* g_out,
                               int64_t lds, int64_t ldg) {
  agp_ctx* ctx = p.ctx;
  for (const agp_pathwise::Lat& a : p.lat)
    if (a.kind == AGP_K_EXPONENTIAL) {
      ctx->err = "agp_pathwise_eval_grad: ExponentialKernel is not differentiable at zero distance";
      return AGP_ERR_UNSUPPORTED;
    }
  AGPCHK(pw_grad_buffers(p));
  const int64_t slab = p.Sp * p.CH;
  for (int l = 0; l < p.nl; ++l) {
    const agp_pathwise::Lat& a = p.lat[l];
    for (int64_t s = 0; s < nt; s += p.CH) {
      const int64_t nc = std::min<int64_t>(p.CH, nt - s), nq = rup64(nc);
      const double* xs = xt + s * ldx;
      if (f_out) AGPCHK(pw_eval_chunk(p, l, xs, ldx, nc, f_out + ((int64_t)l * p.S) * ldo + s, ldo));
      AGPCHK(pw_features<true>(p, a, xs, ldx, nc));
      hipLaunchKernelGGL(agp::k_pw_dkern, dim3((unsigned)(p.mp / TILE), (unsigned)(nq / TILE)), dim3(256), 0, ctx->stream, xs, ldx, nc,
                         p.D, (const double*)a.scales, (const double*)a.Z, p.m, a.kind, a.variance, p.ws + p.Lp, p.ldw);
      LAUNCHCHK(ctx);
      double* g = g_out + (((int64_t)l * p.S) * lds + s) * ldg;
      for (int64_t d0 = 0; d0 < p.D; d0 += p.GD) {
        const int nd = (int)std::min<int64_t>(p.GD, p.D - d0);
        for (int k = 0; k < nd; ++k) {
          hipLaunchKernelGGL(agp::k_pw_grad_operand, grid1(nq * p.ldw), dim3(256), 0, ctx->stream, (const double*)p.ws, nq, nc, p.Lp,
                             (int64_t)p.L, p.mp, p.m, p.ldw, xs, ldx, p.D, d0 + k, (const double*)a.scales, (const double*)a.omega,
                             (const double*)a.Z, p.ws2);
          LAUNCHCHK(ctx);
          AGPCHK((gemm_nt<double, EPI_STORE>(ctx, a.WV, p.ldw, p.ws2, p.ldw, p.Sp, nq, p.ldw, 0, p.Gs + k * slab, p.CH, nullptr, 0,
                                             nullptr, nullptr, nullptr, 0)));
        }
        hipLaunchKernelGGL(agp::k_pw_grad_scatter, dim3((unsigned)p.S, (unsigned)((nc + 63) / 64)), dim3(256), 0, ctx->stream,
                           (const double*)p.Gs, slab, p.CH, nc, nd, g, lds, ldg, d0);
        LAUNCHCHK(ctx);
      }
    }
  }
  return AGP_OK;
}

// ---- agp_pathwise_maximize (include/agp_hip.h; kernels and the formulation: agp_pathwise.h) ------------------------------------------
constexpr int PW_ASCENT_PT = 16;  // particles per workgroup (measured against 32 and 64)
template <int DQ>
static void pw_ascent_launch(agp_pathwise& p, const agp_pathwise::Lat& a, const double* x0, int64_t ldx0, int shared, int64_t R, int64_t np,
                             const agp_pw_ascent_opts& o, const agp::PwAscentBox& box) {
  hipLaunchKernelGGL((agp::k_pw_ascent<PW_ASCENT_PT, DQ>), dim3((unsigned)((np + PW_ASCENT_PT - 1) / PW_ASCENT_PT)), dim3(256), 0,
                     p.ctx->stream, x0, ldx0, shared, R, np, p.D, (const double*)a.scales, (const double*)a.omega, (const double*)a.phase,
                     (int64_t)p.L, a.amp, (const double*)a.Z, p.m, a.kind, a.variance, (const double*)a.WV, p.ldw, p.Lp, (int)o.steps,
                     o.minimize ? -1.0 : 1.0, o.beta1, o.beta2, o.eps, box, p.mxX, p.mxF);
}
// Every check first, touching nothing; then the particle state (grown if this call has more particles than any before: the one
// place that may wait for the device), one launch of k_pw_ascent, the reduction over the starts if a best_* output is asked for,
// and pitched copies of the state into x_out and f_out.  Nothing here waits for the stream.
static agp_status pw_maximize(agp_pathwise* p, int32_t latent, const double* x0, int64_t ldx0, int64_t R, const agp_pw_ascent_opts* o,
                              double* x_out, int64_t ldxo, double* f_out, int64_t ldf, double* best_x, int64_t ldb, double* best_f,
                              int64_t* best_idx) {
  agp_ctx* ctx = p->ctx;
  const char* who = "agp_pathwise_maximize: ";
  auto invalid = [&](const std::string& what) {
    ctx->err = who + what;
    return AGP_ERR_INVALID;
  };
  if (!x0) return invalid("x0 must be given");
  if (!o) return invalid("opts must be given");
  if (!x_out && !f_out && !best_x && !best_f && !best_idx) return invalid("at least one output must be given");
  if (latent < 0 || latent >= p->nl) return invalid("latent must lie in [0, n_latent)");
  const agp_pathwise::Lat& a = p->lat[latent];
  if (a.kind == AGP_K_EXPONENTIAL) {
    ctx->err = std::string(who) + "ExponentialKernel is not differentiable at zero distance";
    return AGP_ERR_UNSUPPORTED;
  }
  if (p->D > agp::PW_AD) {
    ctx->err = std::string(who) + "D > 64 is not supported (D = " + std::to_string(p->D) + ")";
    return AGP_ERR_UNSUPPORTED;
  }
  if (R < 1 || (int64_t)p->S * R >= ((int64_t)1 << 31)) return invalid("n_starts >= 1 and n_samples * n_starts below 2^31");
  if (ldx0 < p->D) return invalid("ldx0 >= D");
  if (x_out && ldxo < p->D) return invalid("ldxo >= D when x_out is given");
  if (f_out && ldf < R) return invalid("ldf >= n_starts when f_out is given");
  if (best_x && ldb < p->D) return invalid("ldb >= D when best_x is given");
  if (o->steps < 0 || o->steps > 65536) return invalid("steps must lie in [0, 65536]");
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return invalid("0 <= beta1, beta2 < 1");
  if (!(o->eps > 0.0) || !std::isfinite(o->eps)) return invalid("eps must be finite and > 0");
  if (!o->lo_host || !o->hi_host || !o->lr_host) return invalid("lo_host, hi_host and lr_host must be given");
  agp::PwAscentBox box{};
  for (int64_t d = 0; d < p->D; ++d) {
    const double lo = o->lo_host[d], hi = o->hi_host[d], lr = o->lr_host[d];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi))
      return invalid("the bounds must be finite with lo <= hi (dimension " + std::to_string(d) + ")");
    if (!std::isfinite(lr) || !(lr > 0.0)) return invalid("the step sizes must be finite and > 0 (dimension " + std::to_string(d) + ")");
    box.lo[d] = lo, box.hi[d] = hi, box.lr[d] = lr;
  }
  const int64_t np = (int64_t)p->S * R;
  if (np > p->mx_cap) {
    for (double** q : {&p->mxX, &p->mxF})
      if (*q) (void)hipFree(*q), *q = nullptr;  // (waits for what still reads them)
    p->mx_cap = 0;
    AGPCHK(dmalloc(ctx, &p->mxX, np * p->D));
    AGPCHK(dmalloc(ctx, &p->mxF, np));
    p->mx_cap = np;
  }
  const int shared = o->x0_shared ? 1 : 0;
  switch ((p->D + 15) / 16) {
    case 1: pw_ascent_launch<1>(*p, a, x0, ldx0, shared, R, np, *o, box); break;
    case 2: pw_ascent_launch<2>(*p, a, x0, ldx0, shared, R, np, *o, box); break;
    case 3: pw_ascent_launch<3>(*p, a, x0, ldx0, shared, R, np, *o, box); break;
    default: pw_ascent_launch<4>(*p, a, x0, ldx0, shared, R, np, *o, box); break;
  }
  LAUNCHCHK(ctx);
  if (best_x || best_f || best_idx) {
    hipLaunchKernelGGL(agp::k_pw_ascent_best, dim3((unsigned)p->S), dim3(256), 0, ctx->stream, (const double*)p->mxX, (const double*)p->mxF,
                       R, p->D, o->minimize ? -1.0 : 1.0, best_x, ldb, best_f, best_idx);
    LAUNCHCHK(ctx);
  }
  if (x_out)
    HIPCHK(ctx, hipMemcpy2DAsync(x_out, sizeof(double) * ldxo, p->mxX, sizeof(double) * p->D, sizeof(double) * p->D, np,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  if (f_out)
    HIPCHK(ctx, hipMemcpy2DAsync(f_out, sizeof(double) * ldf, p->mxF, sizeof(double) * R, sizeof(double) * R, p->S,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  return AGP_OK;
}
