// agp_blas_host.h -- host launchers of the dense products (agp_linalg.h: syrk_tn, xtx_padded, gemm_nt) and of the kernel matrix
// (agp_cavi.h: launch_kernelmatrix), with the per-context scratch they grow.
#pragma once
#include "agp_cavi.h"
#include "agp_ctx.h"
#include "agp_linalg.h"

// Up to this many C tiles a GEMM / symmetric-product launch uses two k-groups per workgroup (512 threads, two waves per SIMD):
// one four-wave workgroup reaches about half of a CU's MFMA rate, and up to ~4 workgroups per CU the second k-group is worth
// more than the extra tiles in flight (measured, step times with 320 -> 1100: fp32 m = B = 2048 0.821 -> 0.789 ms, fp64 m = B =
// 1536 0.703 -> 0.687 ms, 2048 1.37 -> 1.33 ms; C2's 256 / 136 tiles were below the old limit already).
static constexpr int64_t kg2_limit() { return 1100; }
static constexpr int64_t syrk_kg2_limit() { return kg2_limit(); }
static int ctx_cus(agp_ctx* c) {
  if (c->n_cu <= 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || v <= 0) v = 64;
    c->n_cu = v;
  }
  return c->n_cu;
}
static agp_status ensure_bal_ws(agp_ctx* c, size_t need) {
  if (c->bal_bytes < need) {
    if (c->bal_ws) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->bal_ws);
    }
    c->bal_ws = nullptr;
    c->bal_bytes = 0;
    HIPCHK(c, hipMalloc(&c->bal_ws, need));
    c->bal_bytes = need;
  }
  return AGP_OK;
}

// S = A' diag(w) A (lower tiles mirrored), two k-groups per workgroup when the tile count underfills the chip
template <typename T, int MODE>
static agp_status syrk_tn(agp_ctx* c, const T* A, int64_t lda, int64_t n, int64_t Kdim, const T* w, int lower_a, T* out,
                          int64_t ldo, T* eta2, const T* Kinv, int64_t ldm, T lr, const T* rvec = nullptr,
                          T* eta1 = nullptr, const T* kinv_mu0 = nullptr) {
  // rvec: nt rider workgroups also step eta1 (see k_syrk_tn); a dirty hand-over set of the task-graph Cholesky is refilled by
  // further riders (from the fused step, MODE == SY_ETA2 with rvec, and from the packed statistics of the batch-parallel step,
  // MODE == SY_PACK with rvec, whose riders store t = A' rvec into `eta1` instead of stepping it)
  const int64_t nt = n / TILE, tiles = nt * (nt + 1) / 2, nrider = rvec ? nt : 0;
  T* fillp = nullptr;
  int64_t fused_used = 0, fstride = 0, nfill = 0;
  int fnb = 0;
  // (round 3: any symmetric-product launch refills a dirty set, e.g. X'X behind a factorisation with its inverse: the inline refill
  //  in front of the NEXT task graph was a 6 us launch of its own on the hyper-parameter iteration's path)
  if (c->h_dirty[0].on && c->htype == (int)sizeof(T) && out != nullptr) {
    fillp = (T*)c->hset[0];
    fused_used = c->h_dirty[0].used;
    fstride = c->h_dirty[0].stride;
    fnb = c->h_dirty[0].nb;
    nfill = 96;
    c->h_dirty[0].on = false;
  }
  // up to 160 tiles (C2: 136 on 256 CUs, one workgroup per CU) four k-groups: 16 waves per CU instead of 8 -- 58 -> 52 us at C2
  // (step 0.379 -> 0.3735 ms)
  const int kg = (tiles <= 160 && Kdim >= 8 * BK) ? 4 : (tiles <= syrk_kg2_limit() && Kdim >= 4 * BK) ? 2 : 1;
  const int64_t grid = tiles + nrider + nfill;
  if (kg == 4)
    hipLaunchKernelGGL((k_syrk_tn<T, MODE, 4>), dim3((unsigned)grid), dim3(4 * NTHREADS), 0, c->stream, A, lda, Kdim, w,
                       lower_a, out, ldo, eta2, Kinv, ldm, lr, tiles, rvec, eta1, kinv_mu0, nrider, fillp, fused_used, fstride,
                       fnb);
  else if (kg == 2)
    hipLaunchKernelGGL((k_syrk_tn<T, MODE, 2>), dim3((unsigned)grid), dim3(2 * NTHREADS), 0, c->stream, A, lda, Kdim, w,
                       lower_a, out, ldo, eta2, Kinv, ldm, lr, tiles, rvec, eta1, kinv_mu0, nrider, fillp, fused_used, fstride,
                       fnb);
  else
    hipLaunchKernelGGL((k_syrk_tn<T, MODE, 1>), dim3((unsigned)grid), dim3(NTHREADS), 0, c->stream, A, lda, Kdim, w,
                       lower_a, out, ldo, eta2, Kinv, ldm, lr, tiles, rvec, eta1, kinv_mu0, nrider, fillp, fused_used, fstride,
                       fnb);
  LAUNCHCHK(c);
  return AGP_OK;
}

// out = X' X for lower-triangular X  (A^-1 from its inverse Cholesky factor): the symmetric product with the k range of every
// tile starting at its first row, k-groups chosen like everywhere else (it ran with one k-group on 136 tiles: 60 us at m = 1024)
// Round 4: from 8 block rows on, the balanced form (k_xtx_bal: units of at most ch k-blocks, partial tiles added by the last arriver
// in unit order): 42 -> ~15 us at m = 1024 (below 8 block rows the one-workgroup-per-tile product stays).
// (Dg ...: log det from the diagonal factors rides on the reduction launch; *rider_done says whether it did)
template <typename T>
static agp_status xtx_padded(agp_ctx* c, const T* X, int64_t ld, int64_t n, T* out, int64_t ldo, const T* Dg = nullptr,
                             int64_t nvalid = 0, double* ld_out = nullptr, int32_t* status = nullptr, bool* rider_done = nullptr) {
  if (rider_done) *rider_done = false;
  const int64_t nt = n / TILE;
  if (nt < 8)
    return syrk_tn<T, SY_STORE>(c, X, ld, n, n, (const T*)nullptr, 1, out, ldo, (T*)nullptr, (const T*)nullptr, (int64_t)0, T(0));
  const int ch = (int)std::max<int64_t>(2, (nt + XTX_MAXU - 1) / XTX_MAXU);  // at most XTX_MAXU units per tile
  const int64_t nunits = xtx_bal_units(nt, ch), ntri = nt * (nt + 1) / 2;
  AGPCHK(ensure_bal_ws(c, sizeof(T) * (size_t)nunits * TILE * TILE));
  T* fillp = nullptr;
  int64_t fused_used = 0, fstride = 0, nfill = 0;
  int fnb = 0;
  if (c->h_dirty[0].on && c->htype == (int)sizeof(T)) {  // hand-over refill riders, as in syrk_tn()
    fillp = (T*)c->hset[0];
    fused_used = c->h_dirty[0].used;
    fstride = c->h_dirty[0].stride;
    fnb = c->h_dirty[0].nb;
    nfill = 96;
    c->h_dirty[0].on = false;
  }
  hipLaunchKernelGGL((k_xtx_bal<T, 1>), dim3((unsigned)(nunits + nfill)), dim3(NTHREADS), 0, c->stream, X, ld, n, out, ldo,
                       (T*)c->bal_ws, ch, nunits, fillp, fused_used, fstride, fnb);
  const bool rider = Dg != nullptr && ld_out != nullptr;
  hipLaunchKernelGGL((k_xtx_bal_reduce<T>), dim3((unsigned)(ntri + (rider ? 1 : 0))), dim3(NTHREADS), 0, c->stream, n, out, ldo,
                     (const T*)c->bal_ws, ch, Dg, nvalid, ld_out, status);
  LAUNCHCHK(c);
  if (rider && rider_done) *rider_done = true;
  return AGP_OK;
}

template <typename T, int EPI>
static agp_status gemm_nt(agp_ctx* c, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t M, int64_t N, int64_t K,
                          int tri_b, T* C, int64_t ldc, const T* E, int64_t lde, const T* v, T* p0, T* p1,
                          int64_t ldp, const HkArgs<T>* hk = nullptr) {
  dim3 g((unsigned)(N / TILE), (unsigned)(M / TILE));
  const HkArgs<T> hka = hk ? *hk : HkArgs<T>{};  // (EPI_HK only)
  // round 6: 128 x 64 C tiles (k_gemm_nt_tall) for the large fp64 products -- more 64-tiles than two k-groups are used for (C5's
  // 4096-tile kappa GEMM).  AGP_GEMM_TALL=0 / 1 forces (1: wherever the shape allows, M a multiple of 128).
  if constexpr (EPI == EPI_STORE || EPI == EPI_KAPPA) {
    static const int tall = []() {
      const char* e = getenv("AGP_GEMM_TALL");
      return e ? (e[0] == '0' ? 0 : 1) : -1;
    }();
    const bool big = (N / TILE) * (M / TILE) > kg2_limit();
    if (M % (2 * TILE) == 0 && K >= BK && (tall == 1 || (tall < 0 && big && sizeof(T) == 8))) {
      dim3 gt((unsigned)(N / TILE), (unsigned)(M / (2 * TILE)));
      hipLaunchKernelGGL((k_gemm_nt_tall<T, EPI>), gt, dim3(NTHREADS), 0, c->stream, A, lda, B, ldb, K, tri_b, C, ldc, E, lde, p0, p1,
                         ldp);
      LAUNCHCHK(c);
      return AGP_OK;
    }
  }
  // fewer tiles than ~1.25 waves of CUs: two k-groups per workgroup (2 waves per SIMD) instead of idle SIMD slots
  if ((N / TILE) * (M / TILE) <= kg2_limit() && K >= 4 * BK)
    hipLaunchKernelGGL((k_gemm_nt<T, EPI, 2>), g, dim3(2 * NTHREADS), 0, c->stream, A, lda, B, ldb, K, tri_b, C, ldc, E,
                       lde, v, p0, p1, ldp, hka);
  else
    hipLaunchKernelGGL((k_gemm_nt<T, EPI, 1>), g, dim3(NTHREADS), 0, c->stream, A, lda, B, ldb, K, tri_b, C, ldc, E, lde,
                       v, p0, p1, ldp, hka);
  LAUNCHCHK(c);
  return AGP_OK;
}

// kernelmatrix launch: the MFMA form (k_kernelmatrix_mma) up to D = KMM_MAXD, the direct-difference VALU kernel beyond (or with
// AGP_KERNELMATRIX_VALU=1).  Same arguments as the kernels; `cgroups` = number of column groups a fused row-dot is split into
// (<= 0: one group per column tile, like the VALU kernel; 1: the whole row in one workgroup -- streaming prediction).  Returns
// the number of partial slices the row-dot consumer has to sum.
// The MFMA kernel reads the Y side as ready-made tiles (scaled, zero-padded, with squared norms: k_scale_rows).  Callers whose Y
// is a latent's inducing points pass the cached copy (ysc / ysn, see Svgp::ensure_zsc); otherwise the copy is made here into a
// per-context scratch on the same stream (c may be null only together with a cached copy).
static inline int kmm_dp(int64_t D) { return (int)((D + 7) / 8 * 8); }
static inline bool kmm_usable(int64_t D) {
  static const bool force_valu = []() {
    const char* e = getenv("AGP_KERNELMATRIX_VALU");
    return e && e[0] == '1';
  }();
  return D <= KMM_MAXD && !force_valu;
}
template <typename T>
static int launch_kernelmatrix(agp_ctx* c, hipStream_t stream, const T* X, int64_t ldx, const int64_t* idx, int64_t n, const T* Y,
                               int64_t ldy, int64_t p, int64_t D, const T* scales, int kind, T variance, T* out, int64_t ldo,
                               int64_t n_out, int64_t p_out, int sym, T diag_add, const T* alpha, T* part, int64_t ldp,
                               int64_t cgroups = 0, const T* ysc = nullptr, const T* ysn = nullptr) {
  const int64_t nct = (p_out + TILE - 1) / TILE, nrt = (n_out + TILE - 1) / TILE;
  if (!kmm_usable(D)) {
    hipLaunchKernelGGL((k_kernelmatrix<T>), dim3((unsigned)nct, (unsigned)nrt), dim3(NTHREADS), 0, stream, X, ldx, idx, n, Y, ldy, p,
                       D, scales, kind, variance, out, ldo, n_out, p_out, sym, diag_add, alpha, part, ldp);
    return (int)nct;
  }
  const int Dp = kmm_dp(D);
  const int64_t p_pad = nct * TILE;
  if (!ysc) {
    const size_t need = sizeof(T) * (size_t)(p_pad * Dp + p_pad);
    if (c->kmm_bytes < need) {
      if (c->kmm_scratch) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(c->kmm_scratch);
      }
      c->kmm_scratch = nullptr;
      c->kmm_bytes = 0;
      if (hipMalloc(&c->kmm_scratch, need + need / 4) != hipSuccess) return -1;
      c->kmm_bytes = need + need / 4;
    }
    T* sc0 = (T*)c->kmm_scratch;
    hipLaunchKernelGGL((k_scale_rows<T>), dim3((unsigned)((p_pad + 3) / 4)), dim3(256), 0, stream, Y, ldy, p, p_pad, D, Dp, scales, sc0,
                       sc0 + p_pad * Dp);
    ysc = sc0;
    ysn = sc0 + p_pad * Dp;
  }
  const size_t sh = kmm_smem_bytes<T>(Dp);
  const int64_t groups = cgroups <= 0 ? nct : std::min<int64_t>(cgroups, nct);
  const int64_t ctiles = (nct + groups - 1) / groups;
  const int64_t g_eff = (nct + ctiles - 1) / ctiles;
  const dim3 grid((unsigned)g_eff, (unsigned)nrt);
#define AGP_KMM_LAUNCH(KIND)                                                                                                  \
  do {                                                                                                                        \
    if (sh > 64 * 1024) { /* more than 64 KB of dynamic LDS has to be requested once per kernel */                            \
      static size_t asked = 0;                                                                                                \
      if (sh > asked) {                                                                                                       \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kernelmatrix_mma<T, KIND>),                                \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);                                       \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kernelmatrix_mma<T, KIND, 1>),                             \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);                                       \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kernelmatrix_mma<T, KIND, 2>),                             \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);                                       \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kernelmatrix_mma<T, KIND, 3>),                             \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);                                       \
        asked = sh;                                                                                                           \
      }                                                                                                                       \
    }                                                                                                                         \
    if (out == nullptr && !sym && alpha != nullptr)                                                                           \
      hipLaunchKernelGGL((k_kernelmatrix_mma<T, KIND, 1>), grid, dim3(NTHREADS), sh, stream, X, ldx, idx, n, ysc, ysn, p, D, \
                         Dp, scales, variance, out, ldo, n_out, p_out, sym, diag_add, alpha, part, ldp, ctiles);              \
    else if (out != nullptr && !sym && alpha == nullptr)                                                                      \
      hipLaunchKernelGGL((k_kernelmatrix_mma<T, KIND, 2>), grid, dim3(NTHREADS), sh, stream, X, ldx, idx, n, ysc, ysn, p, D, \
                         Dp, scales, variance, out, ldo, n_out, p_out, sym, diag_add, alpha, part, ldp, ctiles);              \
    else if (out != nullptr && sym && alpha == nullptr)                                                                       \
      hipLaunchKernelGGL((k_kernelmatrix_mma<T, KIND, 3>), grid, dim3(NTHREADS), sh, stream, X, ldx, idx, n, ysc, ysn, p, D, \
                         Dp, scales, variance, out, ldo, n_out, p_out, sym, diag_add, alpha, part, ldp, ctiles);              \
    else                                                                                                                      \
      hipLaunchKernelGGL((k_kernelmatrix_mma<T, KIND>), grid, dim3(NTHREADS), sh, stream, X, ldx, idx, n, ysc, ysn, p, D,    \
                         Dp, scales, variance, out, ldo, n_out, p_out, sym, diag_add, alpha, part, ldp, ctiles);              \
  } while (0)
  switch (kind) {
    case AGP_K_SQEXP: AGP_KMM_LAUNCH(K_SQEXP); break;
    case AGP_K_MATERN52: AGP_KMM_LAUNCH(K_MATERN52); break;
    case AGP_K_MATERN32: AGP_KMM_LAUNCH(K_MATERN32); break;
    default: AGP_KMM_LAUNCH(K_EXPONENTIAL); break;
  }
#undef AGP_KMM_LAUNCH
  return (int)g_eff;
}
