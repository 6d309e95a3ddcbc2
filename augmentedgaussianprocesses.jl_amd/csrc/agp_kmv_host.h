// agp_kmv_host.h -- host drivers of the matrix-free kernel operator (agp_kmv.h): the prepared Y side (KmvOp), the launch of
// k_kmv / k_kmv_sum (kmv_apply), the one-shot product behind agp_kernel_matmul (bb_kernel_matmul) and the batched preconditioned
// CG on it with its solver handle (agp_gp_cg: agp_gp_cg_create / _solve / _destroy in agp_capi.hip).  Float64 only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "agp_blas_host.h"
#include "agp_blocks_host.h"
#include "agp_ctx.h"
#include "agp_kmv.h"
#include "agp_select_host.h"

// what agp_greedy_variance refuses in a kernel descriptor, in its words (nullptr: fine)
static const char* kmv_bad_kernel(const agp_kernel_desc* k, int64_t D) {
  if (!k) return "null kernel descriptor";
  if (k->kind < AGP_K_SQEXP || k->kind > AGP_K_EXPONENTIAL || !(k->variance > 0.0) || !std::isfinite(k->variance))
    return "kernel kind 0..3 and a positive finite variance";
  if (k->ard && !k->ard_scales_host) return "ard without ard_scales_host";
  for (int64_t d = 0; d < (k->ard ? D : 1); ++d) {
    const double sc = k->ard ? k->ard_scales_host[d] : k->scale;
    if (!(sc > 0.0) || !std::isfinite(sc)) return "positive finite kernel scales";
  }
  return nullptr;
}

// the Y side of the operator, prepared once per (kernel, Y): scales, k_scale_rows' tiles and squared norms
struct KmvOp {
  int kind = 0, DP = 0;
  double variance = 0.0;
  int64_t D = 0, p = 0;
  double *scales = nullptr, *ysc = nullptr, *ysn = nullptr;
};
static void kmv_release(KmvOp* op) {
  (void)hipFree(op->scales);
  (void)hipFree(op->ysc);
  (void)hipFree(op->ysn);
  op->scales = op->ysc = op->ysn = nullptr;
}
static agp_status kmv_prepare(agp_ctx* ctx, const agp_kernel_desc* k, const double* Y, int64_t p, int64_t ldy, int64_t D,
                              KmvOp* op) {
  op->kind = k->kind, op->variance = k->variance, op->D = D, op->p = p;
  op->DP = D <= 16 ? 16 : D <= 32 ? 32 : 64;
  const int64_t p_pad = rup64(p);
  std::vector<double> hs(D);
  for (int64_t d = 0; d < D; ++d) hs[d] = k->ard ? k->ard_scales_host[d] : k->scale;
  AGPCHK(dmalloc(ctx, &op->scales, D));
  AGPCHK(dmalloc(ctx, &op->ysc, p_pad * op->DP));
  AGPCHK(dmalloc(ctx, &op->ysn, p_pad));
  HIPCHK(ctx, hipMemcpy(op->scales, hs.data(), sizeof(double) * D, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_scale_rows<double>), dim3((unsigned)((p_pad + 3) / 4)), dim3(256), 0, ctx->stream, Y, ldy, p, p_pad, D,
                     op->DP, (const double*)op->scales, op->ysc, op->ysn);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// column groups: as many as fill the chip twice over with the row tiles there are, at most one per column tile and at most 16
// (the slice sum then stays inside the gamma_{p + R} of the documented error bound)
static int kmv_groups(agp_ctx* ctx, int64_t n, int64_t p, int64_t col_groups) {
  const int64_t nct = (p + TILE - 1) / TILE, nrt = (n + TILE - 1) / TILE;
  int64_t g = col_groups > 0 ? col_groups : (2 * (int64_t)ctx_cus(ctx) + nrt - 1) / nrt;
  if (col_groups <= 0) g = std::min<int64_t>(g, 16);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nct));
}

template <int KIND, int DP, int RB>
static void kmv_launch_one(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, int sym,
                           double diag_add, const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
  constexpr size_t sh = kmv_smem_bytes<DP, RB>();
  if constexpr (sh > 64 * 1024) {  // more than 64 KB of dynamic LDS has to be requested once per kernel
    static bool asked = false;
    if (!asked) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmv<KIND, DP, RB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sh);
      asked = true;
    }
  }
  hipLaunchKernelGGL((k_kmv<KIND, DP, RB>), grid, dim3(NTHREADS), sh, st, X, ldx, n, (const double*)op.ysc, (const double*)op.ysn,
                     op.p, op.D, (const double*)op.scales, op.variance, sym, diag_add, V, ldv, r, out, ldo, slice);
}
template <int KIND>
static void kmv_launch_kind(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, int sym,
                            double diag_add, const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
#define AGP_KMV_CASE(DPV)                                                                                          \
  if (r <= 16) kmv_launch_one<KIND, DPV, 1>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice);  \
  else kmv_launch_one<KIND, DPV, 2>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice)
  if (op.DP == 16) { AGP_KMV_CASE(16); }
  else if (op.DP == 32) { AGP_KMV_CASE(32); }
  else { AGP_KMV_CASE(64); }
#undef AGP_KMV_CASE
}

// out (n x r, ldo) = (K(X, Y) + diag_add [sym]) V, enqueued on the context's stream.  groups > 1: ws holds groups * n * r doubles.
static agp_status kmv_apply(agp_ctx* ctx, const KmvOp& op, const double* X, int64_t ldx, int64_t n, int sym, double diag_add,
                            const double* V, int64_t ldv, int r, int groups, double* ws, double* out, int64_t ldo) {
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE));
  double* dst = groups > 1 ? ws : out;
  const int64_t ldd = groups > 1 ? r : ldo, slice = groups > 1 ? n * r : 0;
  switch (op.kind) {
    case AGP_K_SQEXP: kmv_launch_kind<K_SQEXP>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN52: kmv_launch_kind<K_MATERN52>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN32: kmv_launch_kind<K_MATERN32>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    default: kmv_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
  }
  if (groups > 1)
    hipLaunchKernelGGL(k_kmv_sum, grid1(n * r), dim3(256), 0, ctx->stream, (const double*)ws, groups, n, r, out, ldo);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

static agp_status bb_kernel_matmul(agp_ctx* ctx, const agp_kernel_desc* k, const double* x, int64_t n, int64_t ldx, const double* y,
                                   int64_t p, int64_t ldy, int64_t D, int sym, double diag_add, const double* v, int64_t ldv,
                                   int64_t r, int64_t col_groups, double* out, int64_t ldo) {
  KmvOp op;
  double* ws = nullptr;
  agp_status s = kmv_prepare(ctx, k, sym ? x : y, p, sym ? ldx : ldy, D, &op);
  const int groups = kmv_groups(ctx, n, p, col_groups);
  if (s == AGP_OK && groups > 1) s = dmalloc(ctx, &ws, (int64_t)groups * n * r);
  if (s == AGP_OK) s = kmv_apply(ctx, op, x, ldx, n, sym, sym ? diag_add : 0.0, v, ldv, (int)r, groups, ws, out, ldo);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  kmv_release(&op);
  (void)hipFree(ws);
  if (s == AGP_OK && es != hipSuccess) {
    ctx->err = std::string("agp_kernel_matmul : ") + hipGetErrorString(es);
    return AGP_ERR_HIP;
  }
  return s;
}

// ---- batched preconditioned CG on (K(X, X) + sigma2 I) ---------------------------------------------------------------------------
// The handle keeps what is fixed per (X, kernel, sigma2): a copy of X, the prepared operator, and the preconditioner
// P = L L' + sigma2 I of rank k (L: agp_greedy_variance's factor), applied by Woodbury,
//   P^-1 R = (R - L (sigma2 I_k + L'L)^-1 L'R) / sigma2,
// with the k x k matrix inverted once by the Cholesky driver and the three products on the GEMM launchers (padded to tiles of 64).
struct agp_gp_cg {
  agp_ctx* ctx = nullptr;
  int64_t n = 0, np = 0, D = 0, nblk = 0, k = 0, kp = 0;
  double sigma2 = 0.0;
  int groups = 1;
  KmvOp op;
  double *X = nullptr, *ws = nullptr, *L = nullptr, *Lt = nullptr, *Minv = nullptr;
  double *Xv = nullptr, *Rv = nullptr, *Zv = nullptr, *Pv = nullptr, *Qv = nullptr;  // n x 32
  double *Rt = nullptr, *Ct = nullptr, *Wt = nullptr, *Zl = nullptr;                  // 64 x np, 64 x kp, 64 x kp, np x 64
  double *part = nullptr;                                                             // 3 x nblk x 32
  CgScal* sc = nullptr;                                                               // [2]
};
// stop rule of the preconditioner's pivoted Cholesky, relative to the variance: far above the rounding of its residual diagonal
// (about n u), far below any sigma2 a model would use
static constexpr double CG_PRECOND_STOP = 1e-12;

static void cg_release(agp_gp_cg* h) {
  kmv_release(&h->op);
  for (double* q : {h->X, h->ws, h->L, h->Lt, h->Minv, h->Xv, h->Rv, h->Zv, h->Pv, h->Qv, h->Rt, h->Ct, h->Wt, h->Zl, h->part})
    (void)hipFree(q);
  (void)hipFree(h->sc);
  delete h;
}

static agp_status cg_zero(agp_ctx* ctx, double* a, int64_t cnt) {
  hipLaunchKernelGGL(k_cg_zero, grid1(cnt), dim3(256), 0, ctx->stream, a, cnt);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

static agp_status cg_setup(agp_gp_cg* h, const agp_kernel_desc* k, const double* x, int64_t ldx, int64_t rank) {
  agp_ctx* ctx = h->ctx;
  const int64_t n = h->n, np = h->np, D = h->D;
  AGPCHK(dmalloc(ctx, &h->X, n * D));
  HIPCHK(ctx, hipMemcpy2DAsync(h->X, sizeof(double) * D, x, sizeof(double) * ldx, sizeof(double) * D, n, hipMemcpyDeviceToDevice,
                               ctx->stream));
  AGPCHK(kmv_prepare(ctx, k, h->X, n, D, D, &h->op));
  h->groups = kmv_groups(ctx, n, n, 0);
  if (h->groups > 1) AGPCHK(dmalloc(ctx, &h->ws, (int64_t)h->groups * n * KMV_MAXR));
  for (double** q : {&h->Xv, &h->Rv, &h->Zv, &h->Pv, &h->Qv}) AGPCHK(dmalloc(ctx, q, np * CG_LD));
  AGPCHK(dmalloc(ctx, &h->part, 3 * h->nblk * CG_LD));
  AGPCHK(dmalloc(ctx, &h->sc, 2));
  if (rank <= 0) return AGP_OK;
  // the factor: n x m, row-major
  const int64_t m = std::min(rank, n);
  int64_t* idx = nullptr;
  double *z = nullptr, *F = nullptr, *G = nullptr;
  auto drop = [&]() {
    (void)hipFree(idx);
    (void)hipFree(z);
    (void)hipFree(F);
    (void)hipFree(G);
  };
  agp_status s = dmalloc(ctx, &idx, m);
  if (s == AGP_OK) s = dmalloc(ctx, &z, m * D);
  if (s == AGP_OK) s = dmalloc(ctx, &F, n * m);
  int64_t nsel = 0;
  if (s == AGP_OK) s = bb_greedy<double>(ctx, k, h->X, n, D, D, m, CG_PRECOND_STOP, idx, z, D, F, m, nullptr, &nsel);
  if (s != AGP_OK || nsel <= 0) {  // (nothing selected: plain CG)
    drop();
    return s;
  }
  const int64_t kp = rup64(nsel);
  auto build = [&]() -> agp_status {
    AGPCHK(dmalloc(ctx, &h->L, np * kp));
    AGPCHK(dmalloc(ctx, &h->Lt, kp * np));
    AGPCHK(dmalloc(ctx, &G, kp * kp));
    AGPCHK(dmalloc(ctx, &h->Rt, TILE * np));
    AGPCHK(dmalloc(ctx, &h->Ct, TILE * kp));
    AGPCHK(dmalloc(ctx, &h->Wt, TILE * kp));
    AGPCHK(dmalloc(ctx, &h->Zl, np * TILE));
    hipLaunchKernelGGL((k_copy2d_zero<double>), grid2(np, kp), blk2, 0, ctx->stream, (const double*)F, m, n, nsel, h->L, kp, np, kp);
    hipLaunchKernelGGL((k_gv_transpose<double>), dim3((unsigned)((np / 32) * (kp / 32))), dim3(32, 8), 0, ctx->stream,
                       (const double*)h->L, kp, np, kp, h->Lt, np);
    AGPCHK(cg_zero(ctx, h->Rt, TILE * np));
    // sigma2 I + L'L, inverted once
    AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->Lt, np, h->Lt, np, kp, kp, np, 0, G, kp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
    hipLaunchKernelGGL((k_add_diag<double>), grid1(nsel), dim3(256), 0, ctx->stream, G, kp, nsel, h->sigma2);
    LAUNCHCHK(ctx);
    int32_t info = 0;
    int64_t npo = 0;
    return bb_spd_inverse<double>(ctx, G, kp, nsel, nullptr, 0, nullptr, &info, &h->Minv, &npo);
  };
  s = build();
  drop();
  if (s == AGP_OK) h->k = nsel, h->kp = kp;
  return s;
}

// z = P^-1 r and the partials of r . z
static agp_status cg_precond(agp_gp_cg* h, double* part_rz) {
  agp_ctx* ctx = h->ctx;
  const int64_t np = h->np, kp = h->kp;
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->Rt, np, h->Lt, np, TILE, kp, np, 0, h->Ct, kp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->Ct, kp, h->Minv, kp, TILE, kp, kp, 0, h->Wt, kp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->L, kp, h->Wt, kp, np, TILE, kp, 0, h->Zl, TILE, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  hipLaunchKernelGGL(k_cg_precond, dim3((unsigned)h->nblk), dim3(256), 0, ctx->stream, h->n, (const double*)h->Rv,
                     (const double*)h->Zl, (int64_t)TILE, 1.0 / h->sigma2, h->Zv, part_rz);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

static agp_status cg_solve(agp_gp_cg* h, const double* b, int64_t ldb, int r, double tol, int64_t max_iter, int64_t check_every,
                           double* a, int64_t lda, int32_t* iters_host, double* relres_host, int32_t* conv_host) {
  agp_ctx* ctx = h->ctx;
  const int64_t n = h->n, nblk = h->nblk;
  const dim3 g((unsigned)nblk), t(256);
  double *part_pq = h->part, *part_rr = h->part + nblk * CG_LD, *part_rz = part_rr + nblk * CG_LD;
  const bool pre = h->k > 0;
  const double* Z = pre ? h->Zv : nullptr;
  AGPCHK(cg_zero(ctx, h->Pv, h->np * CG_LD));
  hipLaunchKernelGGL(k_cg_update, g, t, 0, ctx->stream, 1, b, ldb, r, n, nblk, (const CgScal*)h->sc, (const double*)part_pq,
                     (const double*)h->Pv, (const double*)h->Qv, h->Xv, h->Rv, pre ? h->Rt : nullptr, h->np, part_rr);
  if (pre) AGPCHK(cg_precond(h, part_rz));
  hipLaunchKernelGGL(k_cg_direction, g, t, 0, ctx->stream, 1, n, nblk, tol * tol, (const CgScal*)(h->sc + 1), h->sc,
                     (const double*)part_pq, (const double*)part_rr, (const double*)part_rz, (const double*)h->Rv, Z, h->Pv);
  LAUNCHCHK(ctx);
  int cur = 0;
  CgScal hs;
  auto read = [&]() -> agp_status {
    HIPCHK(ctx, hipMemcpyAsync(&hs, h->sc + cur, sizeof(CgScal), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_OK;
  };
  for (int64_t it = 0; it < max_iter; ++it) {
    if (it % check_every == 0) {
      AGPCHK(read());
      bool any = false;
      for (int c = 0; c < r; ++c) any = any || hs.active[c];
      if (!any) break;
    }
    AGPCHK(kmv_apply(ctx, h->op, h->X, h->D, n, 1, h->sigma2, h->Pv, CG_LD, r, h->groups, h->ws, h->Qv, CG_LD));
    hipLaunchKernelGGL(k_cg_dot, g, t, 0, ctx->stream, (const double*)h->Pv, (const double*)h->Qv, n, part_pq);
    hipLaunchKernelGGL(k_cg_update, g, t, 0, ctx->stream, 0, b, ldb, r, n, nblk, (const CgScal*)(h->sc + cur), (const double*)part_pq,
                       (const double*)h->Pv, (const double*)h->Qv, h->Xv, h->Rv, pre ? h->Rt : nullptr, h->np, part_rr);
    if (pre) AGPCHK(cg_precond(h, part_rz));
    hipLaunchKernelGGL(k_cg_direction, g, t, 0, ctx->stream, 0, n, nblk, tol * tol, (const CgScal*)(h->sc + cur), h->sc + (cur ^ 1),
                       (const double*)part_pq, (const double*)part_rr, (const double*)part_rz, (const double*)h->Rv, Z, h->Pv);
    LAUNCHCHK(ctx);
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_cg_export, grid1(n * CG_LD), t, 0, ctx->stream, (const double*)h->Xv, n, r, a, lda);
  LAUNCHCHK(ctx);
  AGPCHK(read());
  for (int c = 0; c < r; ++c) {
    if (iters_host) iters_host[c] = hs.iters[c];
    if (relres_host) relres_host[c] = hs.bb[c] > 0.0 ? std::sqrt(hs.rr[c] / hs.bb[c]) : 0.0;
    if (conv_host) conv_host[c] = hs.conv[c];
  }
  return AGP_OK;
}
