// agp_blocks_host.h -- host drivers of the building blocks the C ABI offers without a model handle: kernel matrix
// (bb_kernelmatrix), Cholesky with jitter (pad_spd, bb_potrf), SPD inverse, right solve, and the two diagnostics bb_mfma_peak and
// bb_diag_bench.  Their kernels are in agp_cavi.h, agp_linalg.h and agp_chol.h, launched through agp_blas_host.h and
// agp_chol_host.h; their entry points (agp_kernelmatrix ... agp_dev_diag_bench) are in agp_capi.hip.
#pragma once
#include <string>
#include <vector>

#include "agp_blas_host.h"
#include "agp_cavi.h"
#include "agp_chol_host.h"
#include "agp_ctx.h"
#include "agp_linalg.h"

// ---- building blocks ---------------------------------------------------------------------------------------------
template <typename T>
static agp_status bb_kernelmatrix(agp_ctx* ctx, const agp_kernel_desc* k, const void* x, int64_t n, int64_t ldx,
                                  const int64_t* idx, const void* y, int64_t p, int64_t ldy, int64_t D, void* out,
                                  int64_t ldo) {
  std::vector<T> hs(D);
  for (int64_t d = 0; d < D; ++d) hs[d] = (T)(k->ard ? k->ard_scales_host[d] : k->scale);
  T* ds = nullptr;
  AGPCHK(dmalloc(ctx, &ds, D));
  HIPCHK(ctx, hipMemcpyAsync(ds, hs.data(), sizeof(T) * D, hipMemcpyHostToDevice, ctx->stream));
  const bool sym = (y == nullptr);
  const void* yy = sym ? x : y;
  const int64_t pp = sym ? n : p, ldyy = sym ? ldx : ldy;
  dim3 g((unsigned)((pp + TILE - 1) / TILE), (unsigned)((n + TILE - 1) / TILE));
  const int slices = launch_kernelmatrix<T>(ctx, ctx->stream, (const T*)x, ldx, idx, n, (const T*)yy, ldyy,
                     pp, D, (const T*)ds, k->kind, (T)k->variance, (T*)out, ldo, n, pp, 0, T(0), (const T*)nullptr,
                     (T*)nullptr, (int64_t)0);
  hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(ds);
  if (slices < 0) {  // the scratch for the scaled Y side could not be allocated: nothing was launched
    ctx->err = "agp_kernelmatrix: out of device memory";
    return AGP_ERR_NOMEM;
  }
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    ctx->err = hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  return AGP_OK;
}

// copy A (n x n, lda) into a padded np x np buffer (identity padding), add jitter on the diagonal
template <typename T>
static agp_status pad_spd(agp_ctx* ctx, const void* a, int64_t lda, int64_t n, double jitter, T** Ap, int64_t* np) {
  *np = rup64(n);
  AGPCHK(dmalloc(ctx, Ap, (*np) * (*np)));
  hipLaunchKernelGGL((k_copy2d<T>), grid2(*np, *np), blk2, 0, ctx->stream, (const T*)a, lda, n, n, *Ap, *np, *np, *np,
                     T(1), T(1));
  if (jitter != 0.0)
    hipLaunchKernelGGL((k_add_diag<T>), grid1(n), dim3(256), 0, ctx->stream, *Ap, *np, n, (T)jitter);
  LAUNCHCHK(ctx);
  return AGP_OK;
}

template <typename T>
static agp_status bb_potrf(agp_ctx* ctx, void* a, int64_t lda, int64_t n, double jitter, int32_t* info_host) {
  T *Ap = nullptr, *X = nullptr;
  int32_t* info = nullptr;
  int64_t np;
  AGPCHK(pad_spd<T>(ctx, a, lda, n, jitter, &Ap, &np));
  AGPCHK(dmalloc(ctx, &X, np * np));
  AGPCHK(dmalloc(ctx, &info, 1));
  HIPCHK(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
  T* Dg = nullptr;
  AGPCHK(dmalloc(ctx, &Dg, np * TILE));
  PotrfReq<T> rq{};
  rq.A = Ap, rq.ld = np, rq.n = np, rq.X = X, rq.ldx = np, rq.Dg = Dg, rq.info_dev = info, rq.nvalid = n;
  AGPCHK(potrf_fused<T>(ctx, rq));
  if (chol_use_dag(ctx, np / TILE)) {
    bool lost = false;
    AGPCHK(dag_lost_dependency(ctx, info, &lost));
    if (lost) {  // the input is still intact in `a`: pad it again and factor with per-column launches
      hipLaunchKernelGGL((k_copy2d<T>), grid2(np, np), blk2, 0, ctx->stream, (const T*)a, lda, n, n, Ap, np, np, np, T(1), T(1));
      if (jitter != 0.0) hipLaunchKernelGGL((k_add_diag<T>), grid1(n), dim3(256), 0, ctx->stream, Ap, np, n, (T)jitter);
      AGPCHK(potrf_fused<T>(ctx, rq));
    }
  }
  hipLaunchKernelGGL((k_publish_diag<T>), dim3((unsigned)(np / TILE)), dim3(256), 0, ctx->stream, Ap, np, (const T*)Dg);
  HIPCHK(ctx, hipMemcpy2DAsync(a, sizeof(T) * lda, Ap, sizeof(T) * np, sizeof(T) * n, n, hipMemcpyDeviceToDevice,
                               ctx->stream));
  hipLaunchKernelGGL((k_zero_strict_upper<T>), grid2(n, n), blk2, 0, ctx->stream, (T*)a, lda, n);
  int32_t hinfo = 0;
  HIPCHK(ctx, hipMemcpyAsync(&hinfo, info, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (info_host) *info_host = hinfo;
  (void)hipFree(Ap);
  (void)hipFree(X);
  (void)hipFree(Dg);
  (void)hipFree(info);
  if (hinfo != 0) {
    ctx->err = "PosDefException: matrix is not positive definite; leading minor " + std::to_string(hinfo);
    return AGP_ERR_NOT_POSDEF;
  }
  return AGP_OK;
}

template <typename T>
static agp_status bb_spd_inverse(agp_ctx* ctx, const void* a, int64_t lda, int64_t n, void* ainv, int64_t ldi,
                                 double* logdet_host, int32_t* info_host, T** keep_inv_padded, int64_t* np_out) {
  T *Ap = nullptr, *X = nullptr, *Tw = nullptr, *Inv = nullptr;
  int32_t* info = nullptr;
  double* sc = nullptr;
  int64_t np;
  AGPCHK(pad_spd<T>(ctx, a, lda, n, 0.0, &Ap, &np));
  AGPCHK(dmalloc(ctx, &X, np * np));
  AGPCHK(dmalloc(ctx, &Tw, np * np));
  AGPCHK(dmalloc(ctx, &Inv, np * np));
  AGPCHK(dmalloc(ctx, &info, 1));
  AGPCHK(dmalloc(ctx, &sc, 1));
  HIPCHK(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
  PotrfReq<T> rq{};
  rq.A = Ap, rq.ld = np, rq.n = np, rq.X = X, rq.ldx = np, rq.Dg = Tw, rq.do_x = 1, rq.info_dev = info, rq.nvalid = n;
  AGPCHK(potrf_fused<T>(ctx, rq));
  if (chol_use_dag(ctx, np / TILE)) {
    bool lost = false;
    AGPCHK(dag_lost_dependency(ctx, info, &lost));
    if (lost) {
      hipLaunchKernelGGL((k_copy2d<T>), grid2(np, np), blk2, 0, ctx->stream, (const T*)a, lda, n, n, Ap, np, np, np, T(1), T(1));
      AGPCHK(potrf_fused<T>(ctx, rq));
    }
  }
  AGPCHK(xtx_padded<T>(ctx, X, np, np, Inv, np));
  hipLaunchKernelGGL((k_logdiag_sum<T>), dim3(1), dim3(1024), 0, ctx->stream, (const T*)Tw, n, sc);
  LAUNCHCHK(ctx);
  if (ainv)
    HIPCHK(ctx, hipMemcpy2DAsync(ainv, sizeof(T) * ldi, Inv, sizeof(T) * np, sizeof(T) * n, n, hipMemcpyDeviceToDevice,
                                 ctx->stream));
  int32_t hinfo = 0;
  double hl = 0;
  HIPCHK(ctx, hipMemcpyAsync(&hinfo, info, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(&hl, sc, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (info_host) *info_host = hinfo;
  if (logdet_host) *logdet_host = 2.0 * hl;
  (void)hipFree(Ap);
  (void)hipFree(X);
  (void)hipFree(Tw);
  (void)hipFree(info);
  (void)hipFree(sc);
  if (keep_inv_padded) {
    *keep_inv_padded = Inv;
    *np_out = np;
  } else {
    (void)hipFree(Inv);
  }
  if (hinfo != 0) {
    ctx->err = "PosDefException: matrix is not positive definite; leading minor " + std::to_string(hinfo);
    return AGP_ERR_NOT_POSDEF;
  }
  return AGP_OK;
}

template <typename T>
static agp_status bb_solve_right(agp_ctx* ctx, const void* a, int64_t lda, int64_t n, const void* b, int64_t ldb,
                                 int64_t r, void* x, int64_t ldx, int32_t* info_host) {
  T* Inv = nullptr;
  int64_t np = 0;
  agp_status s = bb_spd_inverse<T>(ctx, a, lda, n, nullptr, 0, nullptr, info_host, &Inv, &np);
  if (s != AGP_OK) {
    if (Inv) (void)hipFree(Inv);
    return s;
  }
  const int64_t rp = rup64(r);
  T *Bp = nullptr, *Xp = nullptr;
  AGPCHK(dmalloc(ctx, &Bp, rp * np));
  AGPCHK(dmalloc(ctx, &Xp, rp * np));
  // zero the padded rows/cols of B (pad_diag = 0) ; padded block of Inv is the identity
  hipLaunchKernelGGL((k_copy2d_zero<T>), grid2(rp, np), blk2, 0, ctx->stream, (const T*)b, ldb, r, n, Bp, np, rp, np);
  LAUNCHCHK(ctx);
  AGPCHK((gemm_nt<T, EPI_STORE>(ctx, Bp, np, Inv, np, rp, np, np, 0, Xp, np, nullptr, 0, nullptr, nullptr, nullptr, 0)));
  HIPCHK(ctx, hipMemcpy2DAsync(x, sizeof(T) * ldx, Xp, sizeof(T) * np, sizeof(T) * n, r, hipMemcpyDeviceToDevice,
                               ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  (void)hipFree(Inv);
  (void)hipFree(Bp);
  (void)hipFree(Xp);
  return AGP_OK;
}

template <typename T>
static agp_status bb_mfma_peak(agp_ctx* ctx, double* tflops) {
  const int blocks = 256 * 8, iters = 4096;
  T* out = nullptr;
  AGPCHK(dmalloc(ctx, &out, (int64_t)blocks * NTHREADS));
  hipEvent_t e0, e1;
  HIPCHK(ctx, hipEventCreate(&e0));
  HIPCHK(ctx, hipEventCreate(&e1));
  hipLaunchKernelGGL((k_mfma_peak<T>), dim3(blocks), dim3(NTHREADS), 0, ctx->stream, out, 64);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
  hipLaunchKernelGGL((k_mfma_peak<T>), dim3(blocks), dim3(NTHREADS), 0, ctx->stream, out, iters);
  HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
  const double flops = (double)blocks * (NTHREADS / 64) * (double)iters * 8.0 * 2.0 * 16 * 16 * 4;
  *tflops = flops / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(out);
  return AGP_OK;
}

template <typename T, int VAR>
static agp_status bb_diag_bench(agp_ctx* ctx, int blocks, int reps, double* us) {
  T *A = nullptr, *out = nullptr;
  int32_t* info = nullptr;
  AGPCHK(dmalloc(ctx, &A, TILE * TILE));
  AGPCHK(dmalloc(ctx, &out, (int64_t)blocks * 2 * TILE * TILE));
  AGPCHK(dmalloc(ctx, &info, 1));
  std::vector<T> h(TILE * TILE);
  for (int i = 0; i < TILE; ++i)
    for (int j = 0; j < TILE; ++j) h[i * TILE + j] = (T)((i == j ? 2.0 : 0.0) + 0.5 / (1.0 + std::abs(i - j)));
  HIPCHK(ctx, hipMemcpy(A, h.data(), sizeof(T) * TILE * TILE, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemset(info, 0, 4));
  hipEvent_t e0, e1;
  HIPCHK(ctx, hipEventCreate(&e0));
  HIPCHK(ctx, hipEventCreate(&e1));
  hipLaunchKernelGGL((k_diag_bench<T, VAR>), dim3(blocks), dim3(CHOL_THREADS), 0, ctx->stream, (const T*)A, out, 2, info);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
  hipLaunchKernelGGL((k_diag_bench<T, VAR>), dim3(blocks), dim3(CHOL_THREADS), 0, ctx->stream, (const T*)A, out, reps, info);
  HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
  *us = ms * 1e3 / reps;
  {  // residuals of block 0 (development aid): |L L' - A|, |X L - I|, strict-upper leakage
     // (VAR 13, "2-level, no X21": the inverse part is [[X11, 0], [L21, X22]] -- |X11 L11 - I|, |X22 L22 - I|, the L21 block exact)
    constexpr bool nox21 = VAR == 13;
    std::vector<T> o(2 * TILE * TILE);
    HIPCHK(ctx, hipMemcpy(o.data(), out, sizeof(T) * 2 * TILE * TILE, hipMemcpyDeviceToHost));
    const T* Lh = o.data();
    const T* Xh = o.data() + TILE * TILE;
    double e1m = 0, e2m = 0, e3m = 0;
    for (int i = 0; i < TILE; ++i)
      for (int j = 0; j < TILE; ++j) {
        double s1 = 0, s2 = 0;
        const int kb = nox21 ? (i / 32) * 32 : 0, ke = nox21 ? kb + 32 : TILE;
        for (int k = 0; k < TILE; ++k) {
          s1 += (double)Lh[i * TILE + k] * (double)Lh[j * TILE + k];
          if (k >= kb && k < ke) s2 += (double)Xh[i * TILE + k] * (double)Lh[k * TILE + j];
        }
        e1m = std::max(e1m, std::abs(s1 - (double)h[i * TILE + j]));
        if (nox21 && i / 32 != j / 32) e2m = std::max(e2m, std::abs((double)Xh[i * TILE + j] - (j < i ? (double)Lh[i * TILE + j] : 0.0)));
        else e2m = std::max(e2m, std::abs(s2 - (i == j ? 1.0 : 0.0)));
        if (j > i) e3m = std::max(e3m, std::abs((double)Lh[i * TILE + j]) + std::abs((double)Xh[i * TILE + j]));
      }
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-4;
    if (!(e1m < tol) || !(e2m < tol) || e3m != 0.0) {
      ctx->err = "diag_bench residual check failed";
      return AGP_ERR_NOT_POSDEF;
    }
  }
  (void)hipFree(A);
  (void)hipFree(out);
  (void)hipFree(info);
  return AGP_OK;
}
