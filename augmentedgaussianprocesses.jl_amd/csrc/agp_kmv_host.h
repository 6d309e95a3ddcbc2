// agp_kmv_host.h -- host drivers of the matrix-free kernel operator (agp_kmv.h): the prepared Y side (KmvOp), the launch of
// k_kmv / k_kmv_sum (kmv_apply), the one-shot product behind agp_kernel_matmul (bb_kernel_matmul) and the batched preconditioned
// CG on it with its solver handle (agp_gp_cg: agp_gp_cg_create / _solve / _destroy in agp_capi.hip), the derivative bilinear form
// (agp_kmv_grad.h: kmv_grad_apply, bb_kernel_bilinear_grad) and what the stochastic log marginal likelihood needs of the solver: the CG
// that reports its Lanczos coefficients (cg_solve_slq), the probes z ~ N(0, P) and log det P.  Float64, except the operator itself,
// which also has a Float32 instance (agp_kmv_f32.h: Kmv32Op, kmv32_prepare, kmv32_apply, bb_kernel_matmul_f32) that the solver handle
// can be switched to (cg_set_operator); its vectors, preconditioner, probes and Lanczos table stay Float64.  The derivative with
// respect to the row points (agp_kmv_dx.h: kmv_dx_apply, kmv_dx_run, bb_kernel_matmul_dx) is Float64 only.  More than 32 and up to 128
// columns go through the wide kernel (agp_kmv_wide.h) inside kmv_apply; cg_set_block sizes the solver handle for 128 columns.
// 65 .. 128 input dimensions: kmv_prepare pads the rows to 96 or 128 and kmv_apply sends the product to k_kmv_hd (agp_kmv_hd.h), up to
// 32 columns, Float64; the Float32 operator, the wide block and the derivative kernels stop at 64 dimensions.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "agp_blas_host.h"
#include "agp_blocks_host.h"
#include "agp_ctx.h"
#include "agp_kmv.h"
#include "agp_kmv_dx.h"
#include "agp_kmv_f32.h"
#include "agp_kmv_grad.h"
#include "agp_kmv_hd.h"
#include "agp_kmv_wide.h"
#include "agp_rand.h"
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
  op->DP = D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : D <= 96 ? 96 : 128;
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

// the wide block (agp_kmv_wide.h): 32 < r <= 128 in one launch, the narrowest of the instances 48, 64, 96, 128 that holds r
template <int KIND, int DP, int RB>
static void kmv_wide_launch_one(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, int sym,
                                double diag_add, const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
  constexpr size_t sh = kmv_smem_bytes<DP, RB>();
  if constexpr (sh > 64 * 1024) {  // more than 64 KB of dynamic LDS has to be requested once per kernel
    static bool asked = false;
    if (!asked) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmv_wide<KIND, DP, RB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sh);
      asked = true;
    }
  }
  hipLaunchKernelGGL((k_kmv_wide<KIND, DP, RB>), grid, dim3(NTHREADS), sh, st, X, ldx, n, (const double*)op.ysc,
                     (const double*)op.ysn, op.p, op.D, (const double*)op.scales, op.variance, sym, diag_add, V, ldv, r, out, ldo, slice);
}
template <int KIND>
static void kmv_wide_launch_kind(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, int sym,
                                 double diag_add, const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
#define AGP_KMVW_CASE(DPV)                                                                                                \
  if (r <= 48) kmv_wide_launch_one<KIND, DPV, 3>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice);      \
  else if (r <= 64) kmv_wide_launch_one<KIND, DPV, 4>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice); \
  else if (r <= 96) kmv_wide_launch_one<KIND, DPV, 6>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice); \
  else kmv_wide_launch_one<KIND, DPV, 8>(st, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, out, ldo, slice)
  if (op.DP == 16) { AGP_KMVW_CASE(16); }
  else if (op.DP == 32) { AGP_KMVW_CASE(32); }
  else { AGP_KMVW_CASE(64); }
#undef AGP_KMVW_CASE
}

// 65 .. 128 input dimensions (agp_kmv_hd.h): r <= 32, the padded width 96 or 128 that kmv_prepare chose
template <int KIND>
static void kmv_hd_launch_kind(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, int sym,
                               double diag_add, const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
#define AGP_KMVHD_ONE(DPV, RBV)                                                                                                     \
  hipLaunchKernelGGL((k_kmv_hd<KIND, DPV, RBV>), grid, dim3(NTHREADS), (kmv_hd_smem_bytes<DPV, RBV>()), st, X, ldx, n,              \
                     (const double*)op.ysc, (const double*)op.ysn, op.p, op.D, (const double*)op.scales, op.variance, sym, diag_add, \
                     V, ldv, r, out, ldo, slice)
#define AGP_KMVHD_CASE(DPV)           \
  if (r <= 16) AGP_KMVHD_ONE(DPV, 1); \
  else AGP_KMVHD_ONE(DPV, 2)
  static_assert(kmv_hd_smem_bytes<128, 2>() <= 64 * 1024, "no instance has to ask for more dynamic LDS than a launch gets");
  if (op.DP == 96) { AGP_KMVHD_CASE(96); }
  else { AGP_KMVHD_CASE(128); }
#undef AGP_KMVHD_CASE
#undef AGP_KMVHD_ONE
}

// out (n x r, ldo) = (K(X, Y) + diag_add [sym]) V, enqueued on the context's stream.  groups > 1: ws holds groups * n * r doubles.
// r <= 32: k_kmv; 32 < r <= 128: k_kmv_wide.  op.D > 64: k_kmv_hd, r <= 32 (the callers refuse more).
static agp_status kmv_apply(agp_ctx* ctx, const KmvOp& op, const double* X, int64_t ldx, int64_t n, int sym, double diag_add,
                            const double* V, int64_t ldv, int r, int groups, double* ws, double* out, int64_t ldo) {
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE));
  double* dst = groups > 1 ? ws : out;
  const int64_t ldd = groups > 1 ? r : ldo, slice = groups > 1 ? n * r : 0;
  if (op.D > KMV_MAXD) switch (op.kind) {
    case AGP_K_SQEXP: kmv_hd_launch_kind<K_SQEXP>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN52: kmv_hd_launch_kind<K_MATERN52>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN32: kmv_hd_launch_kind<K_MATERN32>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    default: kmv_hd_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
  }
  else if (r > KMV_MAXR) switch (op.kind) {
    case AGP_K_SQEXP: kmv_wide_launch_kind<K_SQEXP>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN52: kmv_wide_launch_kind<K_MATERN52>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN32: kmv_wide_launch_kind<K_MATERN32>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
    default: kmv_wide_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, X, ldx, n, op, sym, diag_add, V, ldv, r, dst, ldd, slice); break;
  }
  else switch (op.kind) {
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

// ---- the Float32 operator (agp_kmv_f32.h) -------------------------------------------------------------------------------------------
// Both sides prepared once per (kernel, X, Y): centred by the mean of X, scaled, rounded to Float32, with squared norms.  sym: the Y
// side is the X side (ysc == xsc, not owned twice).
struct Kmv32Op {
  int kind = 0, DP = 0;
  float variance = 0.0f;
  int64_t D = 0, n = 0, p = 0;
  double *scales = nullptr, *mean = nullptr;
  float *xsc = nullptr, *xsn = nullptr, *ysc = nullptr, *ysn = nullptr;
};
static void kmv32_release(Kmv32Op* op) {
  (void)hipFree(op->scales);
  (void)hipFree(op->mean);
  if (op->ysc != op->xsc) {
    (void)hipFree(op->ysc);
    (void)hipFree(op->ysn);
  }
  (void)hipFree(op->xsc);
  (void)hipFree(op->xsn);
  op->scales = op->mean = nullptr;
  op->xsc = op->xsn = op->ysc = op->ysn = nullptr;
}
static std::vector<double> kmv_host_scales(const agp_kernel_desc* k, int64_t D) {
  std::vector<double> hs(D);
  for (int64_t d = 0; d < D; ++d) hs[d] = k->ard ? k->ard_scales_host[d] : k->scale;
  return hs;
}
// TI: the element type of x and y (float: the C ABI with AGP_F32; double: the solver handle's copy of X).  y == nullptr: symmetric.
// hs: the D scales, on the host.
template <typename TI>
static agp_status kmv32_prepare(agp_ctx* ctx, int kind, double variance, const std::vector<double>& hs, const TI* x, int64_t n,
                                int64_t ldx, const TI* y, int64_t p, int64_t ldy, int64_t D, Kmv32Op* op) {
  op->kind = kind, op->variance = (float)variance, op->D = D, op->n = n, op->p = p;
  op->DP = D <= 16 ? 16 : D <= 32 ? 32 : 64;
  const int64_t n_pad = rup64(n), p_pad = rup64(p);
  AGPCHK(dmalloc(ctx, &op->scales, D));
  AGPCHK(dmalloc(ctx, &op->mean, D));
  AGPCHK(dmalloc(ctx, &op->xsc, n_pad * op->DP));
  AGPCHK(dmalloc(ctx, &op->xsn, n_pad));
  HIPCHK(ctx, hipMemcpy(op->scales, hs.data(), sizeof(double) * D, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_kmv32_mean<TI>), dim3((unsigned)D), dim3(256), 0, ctx->stream, x, ldx, n, op->mean);
  hipLaunchKernelGGL((k_kmv32_prep<TI>), dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, ctx->stream, x, ldx, n, n_pad, D, op->DP,
                     (const double*)op->mean, (const double*)op->scales, op->xsc, op->xsn);
  if (!y) {
    op->ysc = op->xsc, op->ysn = op->xsn;
  } else {
    AGPCHK(dmalloc(ctx, &op->ysc, p_pad * op->DP));
    AGPCHK(dmalloc(ctx, &op->ysn, p_pad));
    hipLaunchKernelGGL((k_kmv32_prep<TI>), dim3((unsigned)((p_pad + 3) / 4)), dim3(256), 0, ctx->stream, y, ldy, p, p_pad, D, op->DP,
                       (const double*)op->mean, (const double*)op->scales, op->ysc, op->ysn);
  }
  LAUNCHCHK(ctx);
  return AGP_OK;
}

template <int KIND>
static void kmv32_launch_kind(hipStream_t st, dim3 grid, const Kmv32Op& op, int sym, double diag_add, const void* V, int64_t ldv,
                              int vf32, int r, void* out, int64_t ldo, int64_t slice, int of32, const double* Vdiag, int64_t ldvd) {
#define AGP_KMV32_ONE(DPV, RBV)                                                                                                    \
  hipLaunchKernelGGL((k_kmv32<KIND, DPV, RBV>), grid, dim3(NTHREADS), (kmv32_smem_bytes<DPV, RBV>()), st, (const float*)op.xsc,     \
                     (const float*)op.xsn, op.n, (const float*)op.ysc, (const float*)op.ysn, op.p, op.variance, sym, diag_add, V, \
                     ldv, vf32, r, out, ldo, slice, of32, Vdiag, ldvd)
#define AGP_KMV32_CASE(DPV)            \
  if (r <= 16) AGP_KMV32_ONE(DPV, 1); \
  else AGP_KMV32_ONE(DPV, 2)
  if (op.DP == 16) { AGP_KMV32_CASE(16); }
  else if (op.DP == 32) { AGP_KMV32_CASE(32); }
  else { AGP_KMV32_CASE(64); }
#undef AGP_KMV32_CASE
#undef AGP_KMV32_ONE
}

// out (n x r, ldo; float if of32 else double) = (K(X, Y) + diag_add [sym]) V (p x r, ldv; float if vf32 else double), enqueued on the
// context's stream.  groups > 1: ws holds groups * n * r doubles.  stage (nullable): p * r floats for the rounded copy of a double V.
static agp_status kmv32_apply(agp_ctx* ctx, const Kmv32Op& op, int sym, double diag_add, const void* V, int64_t ldv, int vf32, int r,
                              int groups, double* ws, void* out, int64_t ldo, int of32, float* stage = nullptr) {
  const int64_t n = op.n;
  const double* Vdiag = nullptr;
  const int64_t ldvd = ldv;
  if (!vf32 && stage) {
    hipLaunchKernelGGL(k_kmv32_stage, grid1(op.p * r), dim3(256), 0, ctx->stream, (const double*)V, ldv, op.p, r, stage);
    Vdiag = (const double*)V, V = stage, ldv = r, vf32 = 1;
  }
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE));
  void* dst = groups > 1 ? (void*)ws : out;
  const int64_t ldd = groups > 1 ? r : ldo, slice = groups > 1 ? n * r : 0;
  const int df32 = groups > 1 ? 0 : of32;
  switch (op.kind) {
    case AGP_K_SQEXP: kmv32_launch_kind<K_SQEXP>(ctx->stream, grid, op, sym, diag_add, V, ldv, vf32, r, dst, ldd, slice, df32, Vdiag, ldvd); break;
    case AGP_K_MATERN52: kmv32_launch_kind<K_MATERN52>(ctx->stream, grid, op, sym, diag_add, V, ldv, vf32, r, dst, ldd, slice, df32, Vdiag, ldvd); break;
    case AGP_K_MATERN32: kmv32_launch_kind<K_MATERN32>(ctx->stream, grid, op, sym, diag_add, V, ldv, vf32, r, dst, ldd, slice, df32, Vdiag, ldvd); break;
    default: kmv32_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, op, sym, diag_add, V, ldv, vf32, r, dst, ldd, slice, df32, Vdiag, ldvd); break;
  }
  if (groups > 1)
    hipLaunchKernelGGL(k_kmv32_sum, grid1(n * r), dim3(256), 0, ctx->stream, (const double*)ws, groups, n, r, out, ldo, of32);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// agp_kernel_matmul with AGP_F32: x, y, v and out are float arrays
static agp_status bb_kernel_matmul_f32(agp_ctx* ctx, const agp_kernel_desc* k, const float* x, int64_t n, int64_t ldx, const float* y,
                                       int64_t p, int64_t ldy, int64_t D, int sym, double diag_add, const float* v, int64_t ldv,
                                       int64_t r, int64_t col_groups, float* out, int64_t ldo) {
  Kmv32Op op;
  double* ws = nullptr;
  agp_status s = kmv32_prepare<float>(ctx, k->kind, k->variance, kmv_host_scales(k, D), x, n, ldx, sym ? nullptr : y, p, ldy, D, &op);
  const int groups = kmv_groups(ctx, n, p, col_groups);
  if (s == AGP_OK && groups > 1) s = dmalloc(ctx, &ws, (int64_t)groups * n * r);
  if (s == AGP_OK) s = kmv32_apply(ctx, op, sym, sym ? diag_add : 0.0, v, ldv, 1, (int)r, groups, ws, out, ldo, 1);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  kmv32_release(&op);
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
  double sigma2 = 0.0, logdetM = 0.0;  // logdetM = log det(sigma2 I_k + L'L)
  int groups = 1;
  int block = CG_LD;   // columns per batched solve: 32, or 128 after cg_set_block; the row stride of Xv .. Qv
  int64_t cw = TILE;   // columns the preconditioner's buffers hold (Rt, Ct, Wt rows; Zl's row stride): 64, or 128 at block 128
  KmvOp op;
  Kmv32Op op32;  // the Float32 operator, prepared by cg_set_operator (f32 != 0)
  int f32 = 0;
  float* v32 = nullptr;  // n x 32: the rounded copy of V of a Float32 product
  std::vector<double> scales_host;
  double *X = nullptr, *ws = nullptr, *L = nullptr, *Lt = nullptr, *Minv = nullptr;
  double *Xv = nullptr, *Rv = nullptr, *Zv = nullptr, *Pv = nullptr, *Qv = nullptr;  // np x block
  double *Rt = nullptr, *Ct = nullptr, *Wt = nullptr, *Zl = nullptr;                  // cw x np, cw x kp, cw x kp, np x cw
  double *part = nullptr;                                                             // 3 x (block / 32) panels x nblk x 32
  CgScal* sc = nullptr;                                                               // [block / 32 panels][2]
};
// stop rule of the preconditioner's pivoted Cholesky, relative to the variance: far above the rounding of its residual diagonal
// (about n u), far below any sigma2 a model would use
static constexpr double CG_PRECOND_STOP = 1e-12;

static void cg_release(agp_gp_cg* h) {
  kmv_release(&h->op);
  kmv32_release(&h->op32);
  (void)hipFree(h->v32);
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
  h->scales_host = kmv_host_scales(k, D);
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
    return bb_spd_inverse<double>(ctx, G, kp, nsel, nullptr, 0, &h->logdetM, &info, &h->Minv, &npo);
  };
  s = build();
  drop();
  if (s == AGP_OK) h->k = nsel, h->kp = kp;
  return s;
}

// How many columns a batched solve and a product on the handle take: 32 (as created) or 128.  Everything sized by it is allocated
// anew: the CG vectors (np x block), the partials and the scalar tables (one set per panel of 32 columns), the slices of the
// column-group split, and the preconditioner's transposed residual, its two small products and L's product (cw = 64 or 128
// columns).  The new buffers are allocated FIRST and swapped in only when every one of them is there: a failure leaves the handle
// as it was, valid at its old block.  What is fixed per (X, kernel, sigma2) -- the prepared operator, L, the inverse -- stays.  No
// solve is in flight: every entry point of the handle synchronises before it returns.
static agp_status cg_set_block(agp_gp_cg* h, int block) {
  if (block == h->block) return AGP_OK;
  agp_ctx* ctx = h->ctx;
  const int64_t np = h->np, npan = block / CG_LD, cw = std::max<int64_t>(TILE, block);
  double* nb[11] = {};  // ws, Xv, Rv, Zv, Pv, Qv, part, Rt, Ct, Wt, Zl
  CgScal* nsc = nullptr;
  auto alloc = [&]() -> agp_status {
    if (h->groups > 1) AGPCHK(dmalloc(ctx, &nb[0], (int64_t)h->groups * h->n * block));
    for (int q = 1; q <= 5; ++q) AGPCHK(dmalloc(ctx, &nb[q], np * block));
    AGPCHK(dmalloc(ctx, &nb[6], 3 * npan * h->nblk * CG_LD));
    AGPCHK(dmalloc(ctx, &nsc, 2 * npan));
    if (h->k > 0) {
      AGPCHK(dmalloc(ctx, &nb[7], cw * np));
      AGPCHK(dmalloc(ctx, &nb[8], cw * h->kp));
      AGPCHK(dmalloc(ctx, &nb[9], cw * h->kp));
      AGPCHK(dmalloc(ctx, &nb[10], np * cw));
      AGPCHK(cg_zero(ctx, nb[7], cw * np));  // (Rt: its columns n .. np are never written and enter the first product)
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return AGP_OK;
  };
  const agp_status s = alloc();
  double** cur[11] = {&h->ws, &h->Xv, &h->Rv, &h->Zv, &h->Pv, &h->Qv, &h->part, &h->Rt, &h->Ct, &h->Wt, &h->Zl};
  if (s != AGP_OK) {  // nothing of the handle was touched
    for (double* q : nb) (void)hipFree(q);
    (void)hipFree(nsc);
    return s;
  }
  for (int q = 0; q < 11; ++q) {
    (void)hipFree(*cur[q]);
    *cur[q] = nb[q];
  }
  (void)hipFree(h->sc);
  h->sc = nsc;
  h->block = block, h->cw = cw;
  return AGP_OK;
}

// Which instance of the operator the solves run on.  Float32: the centred Float32 rows of X are prepared from the handle's Float64
// copy (once; kept), and the CG calls k_kmv32 with Float64 V and Out.  Everything else of the handle stays Float64.
static agp_status cg_set_operator(agp_gp_cg* h, int f32) {
  if (f32 && !h->op32.xsc) {
    agp_status s = kmv32_prepare<double>(h->ctx, h->op.kind, h->op.variance, h->scales_host, h->X, h->n, h->D, nullptr, h->n, 0,
                                         h->D, &h->op32);
    if (s == AGP_OK && hipStreamSynchronize(h->ctx->stream) != hipSuccess) s = AGP_ERR_HIP;
    if (s == AGP_OK) s = dmalloc(h->ctx, &h->v32, h->n * KMV_MAXR);
    if (s != AGP_OK) {
      kmv32_release(&h->op32);
      return s;
    }
  }
  h->f32 = f32;
  return AGP_OK;
}

// out (n x r, ldo) = (K + sigma2 I) v (n x r, ldv) on the instance of the operator the handle's solves run on
static agp_status cg_apply(agp_gp_cg* h, const double* v, int64_t ldv, int r, double* out, int64_t ldo) {
  if (h->f32) return kmv32_apply(h->ctx, h->op32, 1, h->sigma2, v, ldv, 0, r, h->groups, h->ws, out, ldo, 0, h->v32);
  return kmv_apply(h->ctx, h->op, h->X, h->D, h->n, 1, h->sigma2, v, ldv, r, h->groups, h->ws, out, ldo);
}

// z = P^-1 r and the partials of r . z, for the first r columns: the three products take 64 columns, or 128 when r > 64 (the GEMM
// launchers work in tiles of 64).  Rows r .. w of Rt may hold residuals of an earlier, wider solve: their products are computed and
// never read (a column of Zl depends on its own row of Rt only) -- up to 63 columns of wasted work, no wrong value.
static agp_status cg_precond(agp_gp_cg* h, int r, double* part_rz) {
  agp_ctx* ctx = h->ctx;
  const int64_t np = h->np, kp = h->kp, w = r <= TILE ? TILE : h->cw;
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->Rt, np, h->Lt, np, w, kp, np, 0, h->Ct, kp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->Ct, kp, h->Minv, kp, w, kp, kp, 0, h->Wt, kp, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->L, kp, h->Wt, kp, np, w, kp, 0, h->Zl, h->cw, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  hipLaunchKernelGGL(k_cg_precond, dim3((unsigned)h->nblk, (unsigned)((r + CG_LD - 1) / CG_LD)), dim3(256), 0, ctx->stream, h->n,
                     (const double*)h->Rv, (const double*)h->Zl, h->cw, 1.0 / h->sigma2, h->Zv, part_rz, (int64_t)h->block);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// What cg_solve_slq asks of cg_solve on top of the solve.  coef: the device table [max_iter][2][block] of (alpha_j, beta_j) per column;
// z0 (n x r, ldz0): the copy of P^-1 b; bpb[c] = b_c' P^-1 b_c (host).  Without a preconditioner P counts as sigma2 I.
struct CgSlq {
  double* coef = nullptr;
  double* z0 = nullptr;
  int64_t ldz0 = 0;
  double bpb[KMV_WIDE_MAXR];
};

static agp_status cg_solve(agp_gp_cg* h, const double* b, int64_t ldb, int r, double tol, int64_t max_iter, int64_t check_every,
                           double* a, int64_t lda, int32_t* iters_host, double* relres_host, int32_t* conv_host,
                           CgSlq* slq = nullptr) {
  agp_ctx* ctx = h->ctx;
  const int64_t n = h->n, nblk = h->nblk, ld = h->block;
  const int npan = (r + CG_LD - 1) / CG_LD;  // panels of 32 columns in use (the y index of the vector kernels' grids)
  const dim3 g((unsigned)nblk, (unsigned)npan), t(256);
  const int64_t pstride = (int64_t)(h->block / CG_LD) * nblk * CG_LD;
  double *part_pq = h->part, *part_rr = h->part + pstride, *part_rz = part_rr + pstride;
  const bool pre = h->k > 0;
  const double* Z = pre ? h->Zv : nullptr;
  double* const coef = slq ? slq->coef : nullptr;
  AGPCHK(cg_zero(ctx, h->Pv, h->np * ld));
  // scalars of panel q: sc[2 q + parity]; the kernels add 2 q themselves
  hipLaunchKernelGGL(k_cg_update, g, t, 0, ctx->stream, 1, b, ldb, r, n, nblk, (const CgScal*)h->sc, (const double*)part_pq,
                     (const double*)h->Pv, (const double*)h->Qv, h->Xv, h->Rv, pre ? h->Rt : nullptr, h->np, part_rr,
                     (double*)nullptr, ld);
  if (pre) AGPCHK(cg_precond(h, r, part_rz));
  hipLaunchKernelGGL(k_cg_direction, g, t, 0, ctx->stream, 1, n, nblk, tol * tol, (const CgScal*)(h->sc + 1), h->sc,
                     (const double*)part_pq, (const double*)part_rr, (const double*)part_rz, (const double*)h->Rv, Z, h->Pv,
                     (double*)nullptr, ld);
  LAUNCHCHK(ctx);
  int cur = 0;
  std::vector<CgScal> hsv(2 * npan);
  auto read = [&]() -> agp_status {
    HIPCHK(ctx, hipMemcpyAsync(hsv.data(), h->sc, sizeof(CgScal) * 2 * npan, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_OK;
  };
  auto hs = [&](int c) -> const CgScal& { return hsv[2 * (c / CG_LD) + cur]; };  // column c's scalars, at index c % 32
  if (slq) {  // z0 = P^-1 b before the first iteration overwrites it, and b' P^-1 b = the first r . z
    hipLaunchKernelGGL(k_cg_export_scaled, grid1(n * ld), t, 0, ctx->stream, (const double*)(pre ? h->Zv : h->Rv), n, r,
                       pre ? 1.0 : 1.0 / h->sigma2, slq->z0, slq->ldz0, ld);
    LAUNCHCHK(ctx);
    AGPCHK(read());
    for (int c = 0; c < r; ++c) slq->bpb[c] = pre ? hs(c).rz[c % CG_LD] : hs(c).rz[c % CG_LD] / h->sigma2;
  }
  for (int64_t it = 0; it < max_iter; ++it) {
    if (it % check_every == 0) {
      AGPCHK(read());
      bool any = false;
      for (int c = 0; c < r; ++c) any = any || hs(c).active[c % CG_LD];
      if (!any) break;
    }
    AGPCHK(cg_apply(h, h->Pv, ld, r, h->Qv, ld));
    hipLaunchKernelGGL(k_cg_dot, g, t, 0, ctx->stream, (const double*)h->Pv, (const double*)h->Qv, n, ld, part_pq);
    hipLaunchKernelGGL(k_cg_update, g, t, 0, ctx->stream, 0, b, ldb, r, n, nblk, (const CgScal*)(h->sc + cur), (const double*)part_pq,
                       (const double*)h->Pv, (const double*)h->Qv, h->Xv, h->Rv, pre ? h->Rt : nullptr, h->np, part_rr,
                       coef ? coef + it * 2 * ld : nullptr, ld);
    if (pre) AGPCHK(cg_precond(h, r, part_rz));
    hipLaunchKernelGGL(k_cg_direction, g, t, 0, ctx->stream, 0, n, nblk, tol * tol, (const CgScal*)(h->sc + cur), h->sc + (cur ^ 1),
                       (const double*)part_pq, (const double*)part_rr, (const double*)part_rz, (const double*)h->Rv, Z, h->Pv,
                       coef ? coef + it * 2 * ld : nullptr, ld);
    LAUNCHCHK(ctx);
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_cg_export, grid1(n * ld), t, 0, ctx->stream, (const double*)h->Xv, n, r, a, lda, ld);
  LAUNCHCHK(ctx);
  AGPCHK(read());
  for (int c = 0; c < r; ++c) {
    const CgScal& q = hs(c);
    const int lc = c % CG_LD;
    if (iters_host) iters_host[c] = q.iters[lc];
    if (relres_host) relres_host[c] = q.bb[lc] > 0.0 ? std::sqrt(q.rr[lc] / q.bb[lc]) : 0.0;
    if (conv_host) conv_host[c] = q.conv[lc];
  }
  return AGP_OK;
}

// ---- the derivative bilinear form (agp_kmv_grad.h) ---------------------------------------------------------------------------------
template <int KIND, int DP, int RB>
static void kmv_grad_launch_one(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, const double* U,
                                int64_t ldu, const double* V, int64_t ldv, int r, const KmvGradW& w, double* part) {
  constexpr size_t sh = kmv_grad_smem_bytes<DP, RB>();
  if constexpr (sh > 64 * 1024) {
    static bool asked = false;
    if (!asked) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmv_grad<KIND, DP, RB>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
      asked = true;
    }
  }
  hipLaunchKernelGGL((k_kmv_grad<KIND, DP, RB>), grid, dim3(NTHREADS), sh, st, X, ldx, n, (const double*)op.ysc,
                     (const double*)op.ysn, op.D, (const double*)op.scales, op.variance, U, ldu, V, ldv, r, w, part);
}
template <int KIND>
static void kmv_grad_launch_kind(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, const double* U,
                                 int64_t ldu, const double* V, int64_t ldv, int r, const KmvGradW& w, double* part) {
#define AGP_KMVG_CASE(DPV)                                                                          \
  if (r <= 16) kmv_grad_launch_one<KIND, DPV, 1>(st, grid, X, ldx, n, op, U, ldu, V, ldv, r, w, part); \
  else kmv_grad_launch_one<KIND, DPV, 2>(st, grid, X, ldx, n, op, U, ldu, V, ldv, r, w, part)
  if (op.DP == 16) { AGP_KMVG_CASE(16); }
  else if (op.DP == 32) { AGP_KMVG_CASE(32); }
  else { AGP_KMVG_CASE(64); }
#undef AGP_KMVG_CASE
}

// out[0] = dvar, out[1 + d] = dscale_d (device, 1 + D doubles) for the r weighted pairs (U[:, c], V[:, c]; w[c]); op is the prepared
// X side (Y = X).  part: groups * row tiles * (1 + D) doubles.  The ExponentialKernel has no derivative at d2 = 0 and is refused by
// the caller.
static agp_status kmv_grad_apply(agp_ctx* ctx, const KmvOp& op, const double* X, int64_t ldx, int64_t n, const double* U, int64_t ldu,
                                 const double* V, int64_t ldv, int r, const KmvGradW& w, int groups, double* part, double* out) {
  const int64_t nrt = (n + TILE - 1) / TILE;
  const dim3 grid((unsigned)groups, (unsigned)nrt);
  switch (op.kind) {
    case AGP_K_SQEXP: kmv_grad_launch_kind<K_SQEXP>(ctx->stream, grid, X, ldx, n, op, U, ldu, V, ldv, r, w, part); break;
    case AGP_K_MATERN52: kmv_grad_launch_kind<K_MATERN52>(ctx->stream, grid, X, ldx, n, op, U, ldu, V, ldv, r, w, part); break;
    default: kmv_grad_launch_kind<K_MATERN32>(ctx->stream, grid, X, ldx, n, op, U, ldu, V, ldv, r, w, part); break;
  }
  hipLaunchKernelGGL(k_kmv_grad_sum, dim3((unsigned)(1 + op.D)), dim3(256), 0, ctx->stream, (const double*)part, groups * nrt,
                     1 + op.D, out);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

static agp_status bb_kernel_bilinear_grad(agp_ctx* ctx, const agp_kernel_desc* k, const double* x, int64_t n, int64_t ldx, int64_t D,
                                          const double* u, int64_t ldu, const double* v, int64_t ldv, int64_t r, const double* w_host,
                                          int64_t col_groups, double* dvar_host, double* dscales_host) {
  KmvOp op;
  double *part = nullptr, *out = nullptr;
  KmvGradW w;
  for (int c = 0; c < KMV_MAXR; ++c) w.w[c] = c < r ? (w_host ? w_host[c] : 1.0) : 0.0;
  std::vector<double> res(1 + D);
  agp_status s = kmv_prepare(ctx, k, x, n, ldx, D, &op);
  const int groups = kmv_groups(ctx, n, n, col_groups);
  if (s == AGP_OK) s = dmalloc(ctx, &part, (int64_t)groups * ((n + TILE - 1) / TILE) * (1 + D));
  if (s == AGP_OK) s = dmalloc(ctx, &out, 1 + D);
  if (s == AGP_OK) s = kmv_grad_apply(ctx, op, x, ldx, n, u, ldu, v, ldv, (int)r, w, groups, part, out);
  hipError_t es = hipSuccess;
  if (s == AGP_OK) es = hipMemcpyAsync(res.data(), out, sizeof(double) * (1 + D), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es2 = hipStreamSynchronize(ctx->stream);
  kmv_release(&op);
  (void)hipFree(part);
  (void)hipFree(out);
  if (s == AGP_OK && (es != hipSuccess || es2 != hipSuccess)) {
    ctx->err = std::string("agp_kernel_bilinear_grad : ") + hipGetErrorString(es != hipSuccess ? es : es2);
    return AGP_ERR_HIP;
  }
  if (s == AGP_OK) {
    *dvar_host = res[0];
    for (int64_t d = 0; d < D; ++d) dscales_host[d] = res[1 + d];
  }
  return s;
}

// ---- the derivative with respect to the row points (agp_kmv_dx.h) ------------------------------------------------------------------
// right-hand sides per column block: 1 for a single column and for paired mode, else 4 (the instances that are built; not tuned)
static int kmv_dx_cb(int r, int paired) { return (paired || r == 1) ? 1 : 4; }
// kmv_groups with the column blocks counted among the workgroups there are
static int kmv_dx_groups(agp_ctx* ctx, int64_t n, int64_t p, int r, int paired, int64_t col_groups) {
  const int cb = kmv_dx_cb(r, paired);
  const int64_t nct = (p + TILE - 1) / TILE, wgs = ((n + TILE - 1) / TILE) * (paired ? 1 : (r + cb - 1) / cb);
  int64_t g = col_groups > 0 ? col_groups : std::min<int64_t>((2 * (int64_t)ctx_cus(ctx) + wgs - 1) / wgs, 16);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nct));
}

template <int KIND, int DP, int CB, bool PAIRED>
static void kmv_dx_launch_one(hipStream_t st, dim3 grid, const double* X, int64_t ldx, int64_t n, const KmvOp& op, const double* V,
                              int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
  constexpr size_t sh = kmv_dx_smem_bytes<DP, CB, PAIRED>();
  if constexpr (sh > 64 * 1024) {  // more than 64 KB of dynamic LDS has to be requested once per kernel
    static bool asked = false;
    if (!asked) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmv_dx<KIND, DP, CB, PAIRED>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
      asked = true;
    }
  }
  hipLaunchKernelGGL((k_kmv_dx<KIND, DP, CB, PAIRED>), grid, dim3(NTHREADS), sh, st, X, ldx, n, (const double*)op.ysc,
                     (const double*)op.ysn, op.p, op.D, (const double*)op.scales, op.variance, V, ldv, r, out, ldo, slice);
}
template <int KIND>
static void kmv_dx_launch_kind(hipStream_t st, dim3 grid, int cb, int paired, const double* X, int64_t ldx, int64_t n, const KmvOp& op,
                               const double* V, int64_t ldv, int r, double* out, int64_t ldo, int64_t slice) {
#define AGP_KMVDX_CASE(DPV)                                                                                \
  if (paired) kmv_dx_launch_one<KIND, DPV, 1, true>(st, grid, X, ldx, n, op, V, ldv, r, out, ldo, slice);  \
  else if (cb == 1) kmv_dx_launch_one<KIND, DPV, 1, false>(st, grid, X, ldx, n, op, V, ldv, r, out, ldo, slice); \
  else kmv_dx_launch_one<KIND, DPV, 4, false>(st, grid, X, ldx, n, op, V, ldv, r, out, ldo, slice)
  if (op.DP == 16) { AGP_KMVDX_CASE(16); }
  else if (op.DP == 32) { AGP_KMVDX_CASE(32); }
  else { AGP_KMVDX_CASE(64); }
#undef AGP_KMVDX_CASE
}

// shared: out (n x r D, ldo)[i][c D + d] = 2 s_d sum_j c_ij V_jc t_ijd; paired (r == n <= 32): out (n x D, ldo)[i][d] with V_ji.  op is the
// prepared column side, V is p x r (ldv).  Enqueued on the context's stream.  groups > 1: ws holds groups * n * (paired ? D : r D)
// doubles.  The ExponentialKernel is refused by the caller.
static agp_status kmv_dx_apply(agp_ctx* ctx, const KmvOp& op, const double* X, int64_t ldx, int64_t n, const double* V, int64_t ldv,
                               int r, int paired, int groups, double* ws, double* out, int64_t ldo) {
  const int cb = kmv_dx_cb(r, paired);
  const int64_t width = (paired ? 1 : r) * op.D;
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE), (unsigned)(paired ? 1 : (r + cb - 1) / cb));
  double* dst = groups > 1 ? ws : out;
  const int64_t ldd = groups > 1 ? width : ldo, slice = groups > 1 ? n * width : 0;
  switch (op.kind) {
    case AGP_K_SQEXP: kmv_dx_launch_kind<K_SQEXP>(ctx->stream, grid, cb, paired, X, ldx, n, op, V, ldv, r, dst, ldd, slice); break;
    case AGP_K_MATERN52: kmv_dx_launch_kind<K_MATERN52>(ctx->stream, grid, cb, paired, X, ldx, n, op, V, ldv, r, dst, ldd, slice); break;
    default: kmv_dx_launch_kind<K_MATERN32>(ctx->stream, grid, cb, paired, X, ldx, n, op, V, ldv, r, dst, ldd, slice); break;
  }
  if (groups > 1)
    hipLaunchKernelGGL(k_kmv_sum, grid1(n * width), dim3(256), 0, ctx->stream, (const double*)ws, groups, n, (int)width, out, ldo);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// prepared column side `op`, workspace of its own, synchronises; `who` names the entry point in a HIP error
static agp_status kmv_dx_run(agp_ctx* ctx, const KmvOp& op, const double* x, int64_t n, int64_t ldx, const double* v, int64_t ldv,
                             int64_t r, int paired, int64_t col_groups, double* out, int64_t ldo, const char* who) {
  double* ws = nullptr;
  agp_status s = AGP_OK;
  const int groups = kmv_dx_groups(ctx, n, op.p, (int)r, paired, col_groups);
  if (groups > 1) s = dmalloc(ctx, &ws, (int64_t)groups * n * (paired ? 1 : r) * op.D);
  if (s == AGP_OK) s = kmv_dx_apply(ctx, op, x, ldx, n, v, ldv, (int)r, paired, groups, ws, out, ldo);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(ws);
  if (s == AGP_OK && es != hipSuccess) {
    ctx->err = std::string(who) + " : " + hipGetErrorString(es);
    return AGP_ERR_HIP;
  }
  return s;
}

static agp_status bb_kernel_matmul_dx(agp_ctx* ctx, const agp_kernel_desc* k, const double* x, int64_t n, int64_t ldx, const double* y,
                                      int64_t p, int64_t ldy, int64_t D, const double* v, int64_t ldv, int64_t r, int paired,
                                      int64_t col_groups, double* out, int64_t ldo) {
  KmvOp op;
  agp_status s = kmv_prepare(ctx, k, y, p, ldy, D, &op);
  if (s == AGP_OK) s = kmv_dx_run(ctx, op, x, n, ldx, v, ldv, r, paired, col_groups, out, ldo, "agp_kernel_matmul_dx");
  else (void)hipStreamSynchronize(ctx->stream);
  kmv_release(&op);
  return s;
}

// ---- stochastic Lanczos quadrature on the CG's own coefficients -------------------------------------------------------------------------
// e1' log(T) e1 for the symmetric tridiagonal T (diagonal d[0 .. m), off-diagonal e[0 .. m - 1)): implicit-shift QL (EISPACK tql2) that
// carries only the first row of the eigenvector matrix.  false: no convergence in 60 sweeps of one eigenvalue, or an eigenvalue <= 0.
static bool slq_e1_log_e1(std::vector<double> d, std::vector<double> e, double* out) {
  const int m = (int)d.size();
  std::vector<double> z(m, 0.0);
  z[0] = 1.0;
  e.resize(m, 0.0);
  for (int l = 0; l < m; ++l) {
    int iter = 0, mm;
    do {
      for (mm = l; mm < m - 1; ++mm) {
        const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
        if (std::fabs(e[mm]) <= 0x1p-53 * dd) break;
      }
      if (mm != l) {
        if (iter++ == 60) return false;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]), r = std::hypot(g, 1.0);
        g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = mm - 1; i >= l; --i) {
          double f = s * e[i];
          const double b = c * e[i];
          e[i + 1] = (r = std::hypot(f, g));
          if (r == 0.0) {
            d[i + 1] -= p;
            e[mm] = 0.0;
            break;
          }
          s = f / r, c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          d[i + 1] = g + (p = s * r);
          g = c * r - b;
          f = z[i + 1];
          z[i + 1] = s * z[i] + c * f;
          z[i] = c * z[i] - s * f;
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[mm] = 0.0;
      }
    } while (mm != l);
  }
  double acc = 0.0;
  for (int k = 0; k < m; ++k) {
    if (!(d[k] > 0.0)) return false;
    acc += z[k] * z[k] * std::log(d[k]);
  }
  *out = acc;
  return true;
}

// cg_solve, plus: z0 = P^-1 b (n x r, ldz0), bpb_host[c] = b_c' P^-1 b_c and quad_host[c] = e1' log(T_c) e1, T_c the Lanczos tridiagonal
// of P^-1/2 (K + sigma2 I) P^-1/2 started at P^-1/2 b_c, built from the CG coefficients of column c:
//   T[0][0] = 1 / alpha_0,  T[j][j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1},  T[j-1][j] = sqrt(beta_{j-1}) / alpha_{j-1}.
// Then b' P^-1/2 log(P^-1/2 (K + sigma2 I) P^-1/2) P^-1/2 b ~= bpb * quad.  A column with no iteration (b = 0) reports 0.
static agp_status cg_solve_slq(agp_gp_cg* h, const double* b, int64_t ldb, int r, double tol, int64_t max_iter, int64_t check_every,
                               double* a, int64_t lda, double* z0, int64_t ldz0, int32_t* iters_host, double* relres_host,
                               int32_t* conv_host, double* bpb_host, double* quad_host) {
  agp_ctx* ctx = h->ctx;
  CgSlq slq;
  slq.z0 = z0, slq.ldz0 = ldz0;
  const int64_t ld = h->block;
  AGPCHK(dmalloc(ctx, &slq.coef, std::max<int64_t>(1, max_iter) * 2 * ld));
  int32_t its[KMV_WIDE_MAXR];
  agp_status s = cg_solve(h, b, ldb, r, tol, max_iter, check_every, a, lda, its, relres_host, conv_host, &slq);
  int64_t mmax = 0;
  for (int c = 0; c < r; ++c) mmax = std::max<int64_t>(mmax, its[c]);
  std::vector<double> co(std::max<int64_t>(1, mmax) * 2 * ld);
  if (s == AGP_OK && mmax > 0 &&
      hipMemcpy(co.data(), slq.coef, sizeof(double) * mmax * 2 * ld, hipMemcpyDeviceToHost) != hipSuccess)
    s = AGP_ERR_HIP;
  (void)hipFree(slq.coef);
  if (s != AGP_OK) return s;
  const bool pre = h->k > 0;
  for (int c = 0; c < r; ++c) {
    const int m = its[c];
    if (iters_host) iters_host[c] = m;
    bpb_host[c] = slq.bpb[c];
    quad_host[c] = 0.0;
    if (m == 0) continue;
    std::vector<double> d(m), e(m > 1 ? m - 1 : 0);
    for (int j = 0; j < m; ++j) {
      const double al = co[(j * 2) * ld + c];
      d[j] = 1.0 / al;
      if (j > 0) {
        const double alp = co[((j - 1) * 2) * ld + c], bep = co[((j - 1) * 2 + 1) * ld + c];
        d[j] += bep / alp;
        e[j - 1] = std::sqrt(bep) / alp;
      }
    }
    double q = 0.0;
    if (!slq_e1_log_e1(d, e, &q)) {
      ctx->err = "agp_gp_cg_solve_slq: the Lanczos tridiagonal of column " + std::to_string(c) + " is not positive definite";
      return AGP_ERR_NOT_POSDEF;
    }
    quad_host[c] = pre ? q : q - std::log(h->sigma2);  // (plain CG runs on K + sigma2 I itself: T = sigma2 T(P^-1/2 . P^-1/2))
  }
  return AGP_OK;
}

// probes z_c ~ N(0, P), P = L L' + sigma2 I: z = L eps1 + sigma eps2.  base (nullable, device): t x (n + k), row c = (eps2 (n), eps1 (k));
// nullptr: the Normal of counter (i, t0 + c, RNG_STREAM_PROBE, 0) under `seed` at entry i of row c (k_mc_normals).  out: n x t, ldo.
enum { RNG_STREAM_PROBE = 0x534C51 };
static agp_status cg_probes(agp_gp_cg* h, int64_t t, const double* base, int64_t ldbase, uint64_t seed, uint32_t t0, double* out,
                            int64_t ldo) {
  agp_ctx* ctx = h->ctx;
  const int64_t n = h->n, w = n + h->k;
  double* E = nullptr;
  auto run = [&]() -> agp_status {
    if (!base) {
      AGPCHK(dmalloc(ctx, &E, t * w));
      for (int64_t c = 0; c < t; ++c)
        hipLaunchKernelGGL(k_mc_normals, grid1(w), dim3(256), 0, ctx->stream, w, seed, t0 + (uint32_t)c, (uint32_t)RNG_STREAM_PROBE,
                           E + c * w);
      LAUNCHCHK(ctx);
      base = E, ldbase = w;
    }
    for (int64_t c0 = 0; c0 < t; c0 += CG_LD) {
      const int r = (int)std::min<int64_t>(CG_LD, t - c0);
      const double* Eb = base + c0 * ldbase;
      if (h->k > 0) {  // Zl = L eps1': eps1 padded into Ct (64 x kp), one GEMM
        hipLaunchKernelGGL((k_copy2d_zero<double>), grid2(TILE, h->kp), blk2, 0, ctx->stream, Eb + n, ldbase, (int64_t)r, h->k, h->Ct,
                           h->kp, (int64_t)TILE, h->kp);
        AGPCHK((gemm_nt<double, EPI_STORE>(ctx, h->L, h->kp, h->Ct, h->kp, h->np, TILE, h->kp, 0, h->Zl, h->cw, nullptr, 0, nullptr,
                                           nullptr, nullptr, 0)));
      }
      hipLaunchKernelGGL(k_cg_probe, grid1(n * CG_LD), dim3(256), 0, ctx->stream, n, r, (const double*)(h->k > 0 ? h->Zl : nullptr),
                         h->cw, std::sqrt(h->sigma2), Eb, ldbase, out + c0, ldo);
      LAUNCHCHK(ctx);
    }
    return AGP_OK;
  };
  agp_status s = run();
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == AGP_OK) s = AGP_ERR_HIP;
  (void)hipFree(E);
  return s;
}
