// agp_path_host.h -- host side of the matrix-free pathwise draw of the exact GP (kernel: agp_path.h; include/agp_hip.h, "MATRIX-FREE
// PATHWISE SAMPLING"): the launch of k_path / k_kmv_sum (path_apply), the draw on a solver handle (path_draw: the tables from the
// generators of agp_pathwise.h, P = Phi(X) W by k_path, R = b - P - sigma E, V = (K + sigma2 I)^-1 R by cg_solve in blocks of 32
// columns) and the evaluation of the paths at any number of points (path_eval: one k_path launch per block of 32 samples).
// The Float32 evaluation (kernel: agp_path_f32.h) is path32_build / path32_apply / path32_eval at the end of this file.
// Decoupled sampling (Wilson et al. 2020):
//   f_s(x) = mean + Phi(x) w_s + K(x, X) v_s ,   v_s = (K + sigma2 I)^-1 (y - mean - Phi(X) w_s - sigma e_s)
// The paths object is a snapshot: it owns copies of the prepared training side, the Omega tiles in the same prepared layout, the phases,
// W, V, E and amp; the solver handle may be destroyed afterwards.  The agp_gp_cg_pathwise_* entry points are in agp_capi.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "agp_kmv_host.h"
#include "agp_path.h"
#include "agp_path_f32.h"
#include "agp_pathwise_host.h"

struct agp_gp_cg_paths {
  agp_ctx* ctx = nullptr;
  int64_t n = 0, D = 0, L = 0, S = 0;
  double amp = 0.0;
  KmvOp op;  // the training side: a copy of the handle's scaled rows, norms and scales
  double *omega = nullptr, *omt = nullptr, *php = nullptr;  // Omega (L x D), its tiles (rup64(L) x DP), the phases (rup64(L))
  double *W = nullptr, *V = nullptr, *E = nullptr;          // L x S, n x S, n x S, dense
  double* ws = nullptr;                                     // the slices of a grouped launch, grown by the call that needs more
  int64_t ws_cap = 0;
  // the Float32 side, built by the first Float32 evaluation (path32_build): the centred training tiles, their norms and the mean of
  // the scaled rows (op32), the Omega tiles (rup64(L) x DP), the compensated phases (rup64(L)), W (L x S) and V (n x S) rounded once
  bool has32 = false;
  Kmv32Op op32;
  float *om32 = nullptr, *ph32 = nullptr, *W32 = nullptr, *V32 = nullptr;
  ~agp_gp_cg_paths() {
    kmv_release(&op);
    kmv32_release(&op32);
    for (float* q : {om32, ph32, W32, V32}) (void)hipFree(q);
    for (double* q : {omega, omt, php, W, V, E, ws}) (void)hipFree(q);
  }
};

// kmv_groups over the concatenated list of nct column tiles
static int path_groups(agp_ctx* ctx, int64_t n, int64_t nct, int64_t col_groups) {
  const int64_t nrt = (n + TILE - 1) / TILE;
  int64_t g = col_groups > 0 ? col_groups : std::min<int64_t>((2 * (int64_t)ctx_cus(ctx) + nrt - 1) / nrt, 16);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nct));
}
static agp_status path_ws(agp_gp_cg_paths& p, int64_t cnt) {
  if (cnt <= p.ws_cap) return AGP_OK;
  (void)hipFree(p.ws);  // (waits for what still reads it)
  p.ws = nullptr, p.ws_cap = 0;
  AGPCHK(dmalloc(p.ctx, &p.ws, cnt));
  p.ws_cap = cnt;
  return AGP_OK;
}

// what one launch multiplies: the feature segment (L rows of W) and the training segment (np rows of V); either may be empty
struct PathArgs {
  const double *X, *W, *V;
  int64_t ldx, n, L, ldw, np, ldv, ldo, slice;
  int r;
  double* out;
};
template <int KIND, int DP, int RB>
static void path_launch_one(hipStream_t st, dim3 grid, const agp_gp_cg_paths& p, const PathArgs& a) {
  constexpr size_t sh = agp::kmv_smem_bytes<DP, RB>();
  if constexpr (sh > 64 * 1024) {  // more than 64 KB of dynamic LDS has to be requested once per kernel
    static bool asked = false;
    if (!asked) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&agp::k_path<KIND, DP, RB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sh);
      asked = true;
    }
  }
  hipLaunchKernelGGL((agp::k_path<KIND, DP, RB>), grid, dim3(NTHREADS), sh, st, a.X, a.ldx, a.n, (const double*)p.omt,
                     (const double*)p.php, a.L, p.amp, a.W, a.ldw, (const double*)p.op.ysc, (const double*)p.op.ysn, a.np, a.V, a.ldv,
                     p.D, (const double*)p.op.scales, p.op.variance, a.r, a.out, a.ldo, a.slice);
}
template <int KIND>
static void path_launch_kind(hipStream_t st, dim3 grid, const agp_gp_cg_paths& p, const PathArgs& a) {
#define AGP_PATH_CASE(DPV)                                     \
  if (a.r <= 16) path_launch_one<KIND, DPV, 1>(st, grid, p, a); \
  else path_launch_one<KIND, DPV, 2>(st, grid, p, a)
  if (p.op.DP == 16) { AGP_PATH_CASE(16); }
  else if (p.op.DP == 32) { AGP_PATH_CASE(32); }
  else { AGP_PATH_CASE(64); }
#undef AGP_PATH_CASE
}
// out (n x r, ldo) = Phi(x) W [L rows] + K(x, X) V [np rows: 0 or the draw's n], enqueued on the context's stream
static agp_status path_apply(agp_gp_cg_paths& p, const double* x, int64_t ldx, int64_t n, int64_t L, const double* W, int64_t np,
                             const double* V, int64_t ld, int r, int64_t col_groups, double* out, int64_t ldo) {
  agp_ctx* ctx = p.ctx;
  const int groups = path_groups(ctx, n, (L + TILE - 1) / TILE + (np + TILE - 1) / TILE, col_groups);
  if (groups > 1) AGPCHK(path_ws(p, (int64_t)groups * n * r));
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE));
  PathArgs a{x, W, V, ldx, n, L, ld, np, ld, groups > 1 ? (int64_t)r : ldo, groups > 1 ? n * r : 0, r, groups > 1 ? p.ws : out};
  switch (p.op.kind) {
    case AGP_K_SQEXP: path_launch_kind<K_SQEXP>(ctx->stream, grid, p, a); break;
    case AGP_K_MATERN52: path_launch_kind<K_MATERN52>(ctx->stream, grid, p, a); break;
    case AGP_K_MATERN32: path_launch_kind<K_MATERN32>(ctx->stream, grid, p, a); break;
    default: path_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, p, a); break;
  }
  if (groups > 1)
    hipLaunchKernelGGL(agp::k_kmv_sum, grid1(n * r), dim3(256), 0, ctx->stream, (const double*)p.ws, groups, n, r, out, ldo);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// the argument limits of the draw (those of agp_svgp_pathwise_draw with m = n), by name; touches nothing
static agp_status path_check_draw(agp_ctx* ctx, int64_t n, int64_t D, int64_t L, int64_t S, int64_t t) {
  const char* who = "agp_gp_cg_pathwise_draw";
  AGPCHK(pw_check_spectral(ctx, who, D, L, t));
  if (S < 1 || S > PW_MAX) {
    ctx->err = std::string(who) + ": n_samples must lie in [1, 65536] (got " + std::to_string(S) + ")";
    return AGP_ERR_INVALID;
  }
  if (L * S > PW_CTR_MAX || n * S > PW_CTR_MAX) {
    ctx->err = std::string(who) + ": n_features * n_samples and n * n_samples must stay below 2^32 (counter words of W and E)";
    return AGP_ERR_INVALID;
  }
  return AGP_OK;
}

// The draw on the handle h; b = y - mean (n values, device).  Tables: latent 0's streams, the counters of the exact-GP draw with m = n.
static agp_status path_draw(agp_gp_cg* h, const double* b, int64_t L, int64_t S, uint64_t seed, int64_t t, double tol,
                            int64_t max_iter, int64_t check_every, int32_t* iters_host, double* relres_host, int32_t* conv_host,
                            agp_gp_cg_paths* p) {
  agp_ctx* ctx = h->ctx;
  const int64_t n = h->n, np = h->np, D = h->D, Lp = rup64(L);
  p->ctx = ctx, p->n = n, p->D = D, p->L = L, p->S = S;
  p->amp = std::sqrt(2.0 * h->op.variance / (double)L);
  p->op.kind = h->op.kind, p->op.DP = h->op.DP, p->op.variance = h->op.variance, p->op.D = D, p->op.p = n;
  const int DP = p->op.DP;
  AGPCHK(dmalloc(ctx, &p->op.scales, D));
  AGPCHK(dmalloc(ctx, &p->op.ysc, np * DP));
  AGPCHK(dmalloc(ctx, &p->op.ysn, np));
  AGPCHK(dmalloc(ctx, &p->omega, L * D));
  AGPCHK(dmalloc(ctx, &p->omt, Lp * DP));
  AGPCHK(dmalloc(ctx, &p->php, Lp));
  AGPCHK(dmalloc(ctx, &p->W, L * S));
  AGPCHK(dmalloc(ctx, &p->V, n * S));
  AGPCHK(dmalloc(ctx, &p->E, n * S));
  HIPCHK(ctx, hipMemcpyAsync(p->op.scales, h->op.scales, sizeof(double) * D, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(p->op.ysc, h->op.ysc, sizeof(double) * np * DP, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(p->op.ysn, h->op.ysn, sizeof(double) * np, hipMemcpyDeviceToDevice, ctx->stream));
  // Omega and the phases; the phases' padding up to the tile is zero
  AGPCHK(pw_spectral(ctx, p->op.kind, D, L, seed, t, 0, p->omega, p->php));
  if (Lp > L) AGPCHK(cg_zero(ctx, p->php + L, Lp - L));
  hipLaunchKernelGGL(agp::k_path_prep, grid1(Lp * DP), dim3(256), 0, ctx->stream, (const double*)p->omega, L, Lp, D, DP, p->omt);
  hipLaunchKernelGGL(agp::k_pw_table, grid1(L * S), dim3(256), 0, ctx->stream, L, S, L, S, S, (int64_t)1, 1, seed, (uint32_t)t,
                     (uint32_t)(4 + agp::PW_STREAM_W), p->W);
  hipLaunchKernelGGL(agp::k_pw_table, grid1(n * S), dim3(256), 0, ctx->stream, n, S, n, S, S, (int64_t)1, 1, seed, (uint32_t)t,
                     (uint32_t)(4 + agp::PW_STREAM_E), p->E);
  LAUNCHCHK(ctx);
  // R = b - Phi(X) W - sigma E, in place in a buffer of its own; then the solves, one block of the handle's columns at a time
  double* Rm = nullptr;
  AGPCHK(dmalloc(ctx, &Rm, n * S));
  auto run = [&]() -> agp_status {
    for (int64_t c0 = 0; c0 < S; c0 += KMV_MAXR)
      AGPCHK(path_apply(*p, h->X, D, n, L, p->W + c0, 0, nullptr, S, (int)std::min<int64_t>(KMV_MAXR, S - c0), 0, Rm + c0, S));
    hipLaunchKernelGGL(agp::k_path_resid, grid1(n * S), dim3(256), 0, ctx->stream, n, S, b, std::sqrt(h->sigma2), (const double*)p->E,
                       Rm);
    LAUNCHCHK(ctx);
    for (int64_t c0 = 0; c0 < S; c0 += h->block)  // (the handle's block: 32, or 128 after agp_gp_cg_set_block)
      AGPCHK(cg_solve(h, Rm + c0, S, (int)std::min<int64_t>(h->block, S - c0), tol, max_iter, check_every, p->V + c0, S,
                      iters_host ? iters_host + c0 : nullptr, relres_host ? relres_host + c0 : nullptr,
                      conv_host ? conv_host + c0 : nullptr));
    return AGP_OK;
  };
  agp_status s = run();
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == AGP_OK) s = AGP_ERR_HIP;
  (void)hipFree(Rm);
  return s;
}

// out (nt x S, ldo) = Phi(x) W + K(x, X) V: one launch per block of 32 samples (plus the slice sum when grouped); asynchronous
static agp_status path_eval(agp_gp_cg_paths& p, const double* x, int64_t ldx, int64_t nt, int64_t col_groups, double* out,
                            int64_t ldo) {
  for (int64_t c0 = 0; c0 < p.S; c0 += KMV_MAXR)
    AGPCHK(path_apply(p, x, ldx, nt, p.L, p.W + c0, p.n, p.V + c0, p.S, (int)std::min<int64_t>(KMV_MAXR, p.S - c0), col_groups,
                      out + c0, ldo));
  return AGP_OK;
}

// ---- Float32 evaluation (agp_path_f32.h) --------------------------------------------------------------------------------------------
// The Float32 side of the snapshot, from its own Float64 tables; nothing of it exists before the first Float32 evaluation.  The
// training side goes through kmv32_prepare on the SCALED rows (op.ysc, row pitch DP) with unit scales: op32.mean is the mean of the
// scaled rows and op32.xsc = float(sX - mean), which is what k_path32's prologue forms for a test point.  A failure leaves no part
// of it behind.
static agp_status path32_build(agp_gp_cg_paths& p) {
  if (p.has32) return AGP_OK;
  agp_ctx* ctx = p.ctx;
  const int64_t Lp = rup64(p.L);
  auto build = [&]() -> agp_status {
    AGPCHK(kmv32_prepare<double>(ctx, p.op.kind, p.op.variance, std::vector<double>(p.D, 1.0), p.op.ysc, p.n, p.op.DP, nullptr, p.n,
                                 0, p.D, &p.op32));
    AGPCHK(dmalloc(ctx, &p.om32, Lp * p.op.DP));
    AGPCHK(dmalloc(ctx, &p.ph32, Lp));
    AGPCHK(dmalloc(ctx, &p.W32, p.L * p.S));
    AGPCHK(dmalloc(ctx, &p.V32, p.n * p.S));
    hipLaunchKernelGGL(agp::k_path32_prep, dim3((unsigned)((Lp + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)p.omega,
                       (const double*)p.php, p.L, Lp, p.D, p.op.DP, (const double*)p.op32.mean, p.om32, p.ph32);
    hipLaunchKernelGGL(agp::k_kmv32_stage, grid1(p.L * p.S), dim3(256), 0, ctx->stream, (const double*)p.W, p.S, p.L, (int)p.S, p.W32);
    hipLaunchKernelGGL(agp::k_kmv32_stage, grid1(p.n * p.S), dim3(256), 0, ctx->stream, (const double*)p.V, p.S, p.n, (int)p.S, p.V32);
    LAUNCHCHK(ctx);
    return AGP_OK;
  };
  const agp_status s = build();
  if (s != AGP_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    kmv32_release(&p.op32);
    for (float** q : {&p.om32, &p.ph32, &p.W32, &p.V32}) {
      (void)hipFree(*q);
      *q = nullptr;
    }
    return s;
  }
  p.has32 = true;
  return AGP_OK;
}

// what one Float32 launch multiplies: columns c0 .. c0 + r of W32 and V32
struct Path32Args {
  const double* X;
  int64_t ldx, n, c0, ldo, slice;
  int r, of32;
  void* out;
};
template <int KIND>
static void path32_launch_kind(hipStream_t st, dim3 grid, const agp_gp_cg_paths& p, const Path32Args& a) {
#define AGP_PATH32_ONE(DPV, RBV)                                                                                                     \
  hipLaunchKernelGGL((agp::k_path32<KIND, DPV, RBV>), grid, dim3(NTHREADS), (agp::kmv32_smem_bytes<DPV, RBV>()), st, a.X, a.ldx, a.n, \
                     p.D, (const double*)p.op.scales, (const double*)p.op32.mean, (const float*)p.om32, (const float*)p.ph32, p.L,   \
                     (float)p.amp, (const float*)p.W32 + a.c0, p.S, (const float*)p.op32.xsc, (const float*)p.op32.xsn, p.n,         \
                     p.op32.variance, (const float*)p.V32 + a.c0, p.S, a.r, a.out, a.ldo, a.slice, a.of32)
#define AGP_PATH32_CASE(DPV)            \
  if (a.r <= 16) AGP_PATH32_ONE(DPV, 1); \
  else AGP_PATH32_ONE(DPV, 2)
  if (p.op.DP == 16) { AGP_PATH32_CASE(16); }
  else if (p.op.DP == 32) { AGP_PATH32_CASE(32); }
  else { AGP_PATH32_CASE(64); }
#undef AGP_PATH32_CASE
#undef AGP_PATH32_ONE
}
// out (n x r floats, ldo) = Phi(x) W[:, c0 .. c0 + r] + K(x, X) V[:, c0 .. c0 + r] on k_path32, enqueued on the context's stream;
// col_groups as path_apply takes it
static agp_status path32_apply(agp_gp_cg_paths& p, const double* x, int64_t ldx, int64_t n, int64_t c0, int r, int64_t col_groups,
                               float* out, int64_t ldo) {
  agp_ctx* ctx = p.ctx;
  const int groups = path_groups(ctx, n, (p.L + TILE - 1) / TILE + (p.n + TILE - 1) / TILE, col_groups);
  if (groups > 1) AGPCHK(path_ws(p, (int64_t)groups * n * r));
  const dim3 grid((unsigned)groups, (unsigned)((n + TILE - 1) / TILE));
  Path32Args a{x, ldx, n, c0, groups > 1 ? (int64_t)r : ldo, groups > 1 ? n * r : 0, r, groups > 1 ? 0 : 1,
               groups > 1 ? (void*)p.ws : (void*)out};
  switch (p.op.kind) {
    case AGP_K_SQEXP: path32_launch_kind<K_SQEXP>(ctx->stream, grid, p, a); break;
    case AGP_K_MATERN52: path32_launch_kind<K_MATERN52>(ctx->stream, grid, p, a); break;
    case AGP_K_MATERN32: path32_launch_kind<K_MATERN32>(ctx->stream, grid, p, a); break;
    default: path32_launch_kind<K_EXPONENTIAL>(ctx->stream, grid, p, a); break;
  }
  if (groups > 1)
    hipLaunchKernelGGL(agp::k_kmv32_sum, grid1(n * r), dim3(256), 0, ctx->stream, (const double*)p.ws, groups, n, r, (void*)out, ldo, 1);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

// out (nt x S floats, ldo) = Phi(x) W + K(x, X) V: one k_path32 launch per block of 32 samples (plus the slice sum when grouped);
// asynchronous but for the first call, which builds the Float32 side
static agp_status path32_eval(agp_gp_cg_paths& p, const double* x, int64_t ldx, int64_t nt, int64_t col_groups, float* out,
                              int64_t ldo) {
  AGPCHK(path32_build(p));
  for (int64_t c0 = 0; c0 < p.S; c0 += KMV_MAXR)
    AGPCHK(path32_apply(p, x, ldx, nt, c0, (int)std::min<int64_t>(KMV_MAXR, p.S - c0), col_groups, out + c0, ldo));
  return AGP_OK;
}
