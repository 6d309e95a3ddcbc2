// agp_select_host.h -- host drivers of inducing-point selection: nearest-centre assignment and Lloyd iterations (km_assign,
// km_objective, bb_nearest, bb_kmeans; kernels: agp_kmeans.h) and the greedy conditional-variance selection, a pivoted partial
// Cholesky of K_NN (bb_greedy; kernels: agp_greedy.h).  Their entry points (agp_nearest_center, agp_kmeans, agp_greedy_variance)
// are in agp_capi.hip.
#pragma once
#include <string>
#include <vector>

#include "agp_ctx.h"
#include "agp_greedy.h"
#include "agp_kmeans.h"

// ---- inducing-point selection: nearest-centre assignment and Lloyd iterations (agp_kmeans.h) --------------------------
template <typename T>
static agp_status km_assign(agp_ctx* ctx, const T* x, int64_t n, int64_t ldx, int64_t D, const T* c, int64_t ldc, int64_t m,
                            T* cn, int32_t* labels, T* mind) {
  const int64_t mp = rup64(m);
  const int Dp = (int)((D + 15) / 16 * 16);
  hipLaunchKernelGGL((k_km_cnorm<T>), grid1(mp), dim3(256), 0, ctx->stream, c, ldc, m, mp, D, cn);
  const size_t sh = sizeof(T) * (2 * TILE * (Dp + 2) + 4 * TILE) + sizeof(int) * 2 * TILE;
  if (sh > 64 * 1024)  // gfx950 has 160 KB of LDS per workgroup; more than 64 KB of dynamic LDS has to be requested
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_km_assign<T>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  hipLaunchKernelGGL((k_km_assign<T>), dim3((unsigned)((n + TILE - 1) / TILE)), dim3(NTHREADS), sh, ctx->stream, x, ldx, n, D,
                     Dp, c, ldc, m, mp, (const T*)cn, labels, mind);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

template <typename T>
static agp_status km_objective(agp_ctx* ctx, const T* mind, int64_t n, double* part, double* host) {
  const int nb = 256;
  hipLaunchKernelGGL((k_km_sum_partial<T>), dim3(nb), dim3(256), 0, ctx->stream, mind, n, part);
  hipLaunchKernelGGL(k_km_sum_final, dim3(1), dim3(256), 0, ctx->stream, (const double*)part, nb, part + nb);
  LAUNCHCHK(ctx);
  HIPCHK(ctx, hipMemcpyAsync(host, part + nb, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

template <typename T>
static agp_status bb_nearest(agp_ctx* ctx, const void* x, int64_t n, int64_t ldx, int64_t D, const void* c, int64_t ldc,
                             int64_t m, int32_t* labels, void* mind) {
  if (!x || !c || n <= 0 || m <= 0 || D <= 0 || D > KM_MAXD || ldx < D || ldc < D || (!labels && !mind)) return AGP_ERR_INVALID;
  T* cn = nullptr;
  int32_t* lab = labels;
  T* md = (T*)mind;
  agp_status st = dmalloc(ctx, &cn, rup64(m));
  if (st == AGP_OK && !lab) st = dmalloc(ctx, &lab, n);
  if (st == AGP_OK && !md) st = dmalloc(ctx, &md, n);
  if (st == AGP_OK) {
    st = km_assign<T>(ctx, (const T*)x, n, ldx, D, (const T*)c, ldc, m, cn, lab, md);
    (void)hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(cn);
  if (!labels) (void)hipFree(lab);
  if (!mind) (void)hipFree(md);
  return st;
}

template <typename T>
static agp_status bb_kmeans(agp_ctx* ctx, const void* xv, int64_t n, int64_t ldx, int64_t D, void* cv, int64_t ldc,
                            int64_t m, int max_iter, double tol, int32_t* labels_out, int32_t* counts_out, int32_t* iters,
                            double* objective, int32_t* converged) {
  if (!xv || !cv || n <= 0 || m <= 0 || m > n || D <= 0 || D > KM_MAXD || ldx < D || ldc < D || max_iter < 0)
    return AGP_ERR_INVALID;
  const T* x = (const T*)xv;
  T* c = (T*)cv;
  const int64_t mp = rup64(m);
  const int Dp = (int)((D + 15) / 16 * 16);
  const int nchunks = (int)((n + KM_CHUNK - 1) / KM_CHUNK);
  T *cn = nullptr, *mind = nullptr, *part = nullptr;
  double* red = nullptr;
  int32_t *lab = labels_out, *blist = nullptr, *boff = nullptr;
  if (mp / TILE > KM_MAXTILES) {
    ctx->err = "agp_kmeans: more than 16384 centres";
    return AGP_ERR_UNSUPPORTED;
  }
  auto release = [&]() {  // (hipFree(nullptr) is a no-op: whatever a failed dmalloc left unallocated)
    (void)hipFree(cn);
    (void)hipFree(mind);
    (void)hipFree(part);
    (void)hipFree(red);
    (void)hipFree(blist);
    (void)hipFree(boff);
    if (!labels_out) (void)hipFree(lab);
  };
  agp_status st = dmalloc(ctx, &cn, mp);
  if (st == AGP_OK) st = dmalloc(ctx, &mind, n);
  if (st == AGP_OK) st = dmalloc(ctx, &part, (int64_t)nchunks * mp * (Dp + 16));
  if (st == AGP_OK) st = dmalloc(ctx, &red, 512);
  if (st == AGP_OK) st = dmalloc(ctx, &blist, (int64_t)nchunks * KM_CHUNK);
  if (st == AGP_OK) st = dmalloc(ctx, &boff, (int64_t)nchunks * (KM_MAXTILES + 1));
  if (st == AGP_OK && !lab) st = dmalloc(ctx, &lab, n);
  if (st != AGP_OK) {
    release();
    return st;
  }
  double obj = 0.0, prev = 0.0;
  int it = 0, conv = 0;
  // Clustering.kmeans!: assignments for the seeds, then { centres <- cluster means ; assignments ; |change of cost| < tol }
  st = km_assign<T>(ctx, x, n, ldx, D, c, ldc, m, cn, lab, mind);
  if (st == AGP_OK) st = km_objective<T>(ctx, mind, n, red, &obj);
  while (st == AGP_OK && it < max_iter && !conv) {
    ++it;
    hipLaunchKernelGGL(k_km_bucket, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, (const int32_t*)lab, n,
                       (int)(mp / TILE), blist, boff);
    hipLaunchKernelGGL((k_km_sums<T>), dim3((unsigned)(mp / TILE), (unsigned)nchunks), dim3(NTHREADS), 0, ctx->stream, x, ldx, n,
                       D, Dp, (const int32_t*)lab, mp, (const int32_t*)blist, (const int32_t*)boff, part);
    hipLaunchKernelGGL((k_km_finish<T>), grid1(m * D), dim3(256), 0, ctx->stream, (const T*)part, nchunks, mp, Dp, m, D, c, ldc);
    if (hipGetLastError() != hipSuccess) {
      st = AGP_ERR_HIP;
      break;
    }
    st = km_assign<T>(ctx, x, n, ldx, D, c, ldc, m, cn, lab, mind);
    prev = obj;
    if (st == AGP_OK) st = km_objective<T>(ctx, mind, n, red, &obj);
    if (m == 1 || std::abs(obj - prev) < tol) conv = 1;
  }
  if (st == AGP_OK && counts_out) {  // the histogram of the final assignment (also the only one, for max_iter = 0)
    if (hipMemsetAsync(counts_out, 0, sizeof(int32_t) * (size_t)m, ctx->stream) != hipSuccess) st = AGP_ERR_HIP;
    if (st == AGP_OK) {
      hipLaunchKernelGGL(k_km_hist, dim3((unsigned)nchunks), dim3(256), sizeof(int) * (size_t)m, ctx->stream, (const int32_t*)lab, n,
                         (int)m, counts_out);
      if (hipGetLastError() != hipSuccess) st = AGP_ERR_HIP;
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  release();
  if (iters) *iters = it;
  if (objective) *objective = obj;
  if (converged) *converged = conv;
  return st;
}

// ---- inducing-point selection: greedy conditional variance, a pivoted partial Cholesky of K_NN (agp_greedy.h) --------------------
template <typename T>
static agp_status bb_greedy(agp_ctx* ctx, const agp_kernel_desc* k, const void* xv, int64_t n, int64_t ldx, int64_t D, int64_t m,
                            double tol, int64_t* idx_out, void* zv, int64_t ldz, void* factor_out, int64_t ldf, double* trace_out,
                            int64_t* n_selected_host) {
  const T* x = (const T*)xv;
  T* z = (T*)zv;
  const int64_t Np = (n + GV_BLOCK - 1) / GV_BLOCK * GV_BLOCK, nblk = Np / GV_BLOCK;
  double *F = nullptr, *Xt = nullptr, *dres = nullptr, *aux = nullptr;
  GvPart* part = nullptr;
  GvState* st = nullptr;
  auto release = [&]() {
    (void)hipFree(F);
    (void)hipFree(Xt);
    (void)hipFree(dres);
    (void)hipFree(aux);
    (void)hipFree(part);
    (void)hipFree(st);
  };
  // the factor, column-contiguous: 8 n m bytes (n padded to the workgroup)
  if (m > (int64_t)(INT64_MAX / 8) / Np || hipMalloc((void**)&F, sizeof(double) * (size_t)(m * Np)) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "agp_greedy_variance: cannot allocate the factor workspace of " +
               (m > (int64_t)(INT64_MAX / 8) / Np ? std::string("more than 2^63") : std::to_string(8 * m * Np)) + " bytes (8 n m)";
    return AGP_ERR_NOMEM;
  }
  agp_status s = dmalloc(ctx, &Xt, D * Np);
  if (s == AGP_OK) s = dmalloc(ctx, &dres, Np);
  if (s == AGP_OK) s = dmalloc(ctx, &aux, 2 * GV_MAXD + m);  // scales | pivot coordinates | pivot coefficient row
  if (s == AGP_OK) s = dmalloc(ctx, &part, nblk);
  if (s == AGP_OK) s = dmalloc(ctx, &st, 1);
  if (s != AGP_OK) {
    release();
    return s;
  }
  double *scales = aux, *zp = aux + GV_MAXD, *lp = aux + 2 * GV_MAXD;
  std::vector<double> hs(D);
  for (int64_t d = 0; d < D; ++d) hs[d] = k->ard ? k->ard_scales_host[d] : k->scale;
  hipError_t e = hipMemcpyAsync(scales, hs.data(), sizeof(double) * D, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(F, 0, sizeof(double) * (size_t)(m * Np), ctx->stream);  // columns behind an early stop: 0
  if (e == hipSuccess) e = hipMemsetAsync(st, 0, sizeof(GvState), ctx->stream);
  if (e == hipSuccess) {
    const int64_t tiles = ((n + 31) / 32) * ((D + 31) / 32);
    hipLaunchKernelGGL((k_gv_transpose<T>), dim3((unsigned)tiles), dim3(32, 8), 0, ctx->stream, x, ldx, n, D, Xt, Np);
    hipLaunchKernelGGL((k_gv_prefill<T>), grid1(m * D), dim3(256), 0, ctx->stream, m, (int)D, idx_out, z, ldz, trace_out);
    hipLaunchKernelGGL(k_gv_init, dim3((unsigned)nblk), dim3(GV_BLOCK), 0, ctx->stream, n, k->variance, dres, part);
    const double thr = tol * k->variance;
    for (int64_t j = -1; j < m; ++j) {
      if (j >= 0)
        hipLaunchKernelGGL(k_gv_step, dim3((unsigned)nblk), dim3(GV_BLOCK), 0, ctx->stream, (const double*)Xt,
                           (const double*)scales, n, Np, (int)D, (int)k->kind, k->variance, j, F, dres, (const GvState*)st,
                           (const double*)zp, (const double*)lp, part);
      hipLaunchKernelGGL((k_gv_finish<T>), dim3(1), dim3(GV_BLOCK), 0, ctx->stream, (const GvPart*)part, nblk, j, m, thr, x, ldx,
                         (int)D, (const double*)F, Np, st, zp, lp, idx_out, z, ldz, trace_out);
    }
    if (factor_out) {
      const int64_t ft = ((m + 31) / 32) * ((n + 31) / 32);
      hipLaunchKernelGGL((k_gv_transpose<double>), dim3((unsigned)ft), dim3(32, 8), 0, ctx->stream, (const double*)F, Np, m, n,
                         (double*)factor_out, ldf);
    }
    e = hipGetLastError();
  }
  GvState hst{};
  if (e == hipSuccess) e = hipMemcpyAsync(&hst, st, sizeof(GvState), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // the one synchronisation of the call
  release();
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    ctx->err = std::string("agp_greedy_variance : ") + hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  if (n_selected_host) *n_selected_host = hst.nsel;
  return AGP_OK;
}
