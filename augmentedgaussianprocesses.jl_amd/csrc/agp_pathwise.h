// agp_pathwise.h -- device code of pathwise (decoupled) posterior sampling (Wilson et al. 2020; include/agp_hip.h, "PATHWISE
// SAMPLING"): the spectral draw of the random Fourier features, the Normal tables W and E, the feature kernel Phi(x) and the small
// element-wise kernels of the draw.  The products of the draw and of an evaluation are the library's own (gemm_nt, k_gemm_tn).
// Every table entry is a function of (seed, t, stream, index) alone -- streams 4 + 8 l .. 8 + 8 l of latent l -- with log and
// cos 2 pi by the arithmetic of streams 2 and 3 (agp_rand.h), so a host program reproduces Omega, the phases, W and E bit for bit
// (tests/_pathwise_ref.py does).  No kernel here uses scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_rand.h"

namespace agp {

enum { PW_STREAM_Z = 0, PW_STREAM_GAMMA = 1, PW_STREAM_PHASE = 2, PW_STREAM_W = 3, PW_STREAM_E = 4 };  // + 4 + 8 l
constexpr int PW_DC = 32;  // input dimensions staged per pass of the feature kernel

// the Normal of block 0 at counter (i, t, stream, 0): sqrt(-2 log a) cos(2 pi b) by the contracted arithmetic (k_mc_normals)
__device__ __forceinline__ double pw_normal(uint32_t i, uint32_t t, uint32_t stream, uint64_t seed) {
#pragma clang fp contract(off)
  const Philox4 b = philox4x32_10(i, t, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u0 = u53(b.w[0], b.w[1]), u1 = u53(b.w[2], b.w[3]);
  return sqrt(-2.0 * mc_log(u0)) * mc_cos2pi(u1);
}

// The spectral draw: one lane per (j, d).  omega[j][d] = z_jd for the SqExponential kernel, z_jd sqrt(nu / G_j) for the Matern
// family (nu = 5/2, 3/2, 1/2: a Student-t spectrum with 2 nu degrees of freedom), G_j = n_j^2 / 2 - log u_j2 - log u_j3 with as
// many logarithms as nu - 1/2 (Gamma(nu, 1) without rejection).  The lane of d = 0 also writes phase[j] = 2 pi u_j.
__global__ __launch_bounds__(256) void k_pw_spectral(int64_t n, int64_t D, int kind, uint64_t seed, uint32_t t, uint32_t s0,
                                                     double* __restrict__ omega, double* __restrict__ phase) {
#pragma clang fp contract(off)
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint32_t j = (uint32_t)(e / D);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  double w = pw_normal((uint32_t)e, t, s0 + PW_STREAM_Z, seed);
  if (kind != K_SQEXP) {
    const double nu = kind == K_MATERN52 ? 2.5 : (kind == K_MATERN32 ? 1.5 : 0.5);
    const double nj = pw_normal(j, t, s0 + PW_STREAM_GAMMA, seed);
    double g = (nj * nj) * 0.5;
    if (kind != K_EXPONENTIAL) {
      const Philox4 b = philox4x32_10(j, t, s0 + PW_STREAM_GAMMA, 1u, k0, k1);
      g = g - mc_log(u53(b.w[0], b.w[1]));
      if (kind == K_MATERN52) g = g - mc_log(u53(b.w[2], b.w[3]));
    }
    w = w * sqrt(nu / g);
  }
  omega[e] = w;
  if (e - (int64_t)j * D == 0) {
    const Philox4 b = philox4x32_10(j, t, s0 + PW_STREAM_PHASE, 0u, k0, k1);
    phase[j] = 6.283185307179586 * u53(b.w[0], b.w[1]);
  }
}

// A Normal table T[j][s], j < nj, s < S, at counter (j S + s, t, stream, 0), stored at out[j sj + s ss]; the padding up to
// (njp, Sp) is written as zero.  s_fast != 0: consecutive lanes walk s (E, stored nj x S), else j (W, stored transposed).
__global__ __launch_bounds__(256) void k_pw_table(int64_t nj, int64_t S, int64_t njp, int64_t Sp, int64_t sj, int64_t ss, int s_fast,
                                                  uint64_t seed, uint32_t t, uint32_t stream, double* __restrict__ out) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= njp * Sp) return;
  const int64_t j = s_fast ? e / Sp : e % njp, s = s_fast ? e % Sp : e / njp;
  out[j * sj + s * ss] = (j < nj && s < S) ? pw_normal((uint32_t)(j * S + s), t, stream, seed) : 0.0;
}

// dst[r ld + c] = src[r sr + c sc], r < rows, c < cols (the tables as agp_pathwise_get hands them out)
__global__ void k_pw_gather(const double* __restrict__ src, int64_t sr, int64_t sc, int64_t rows, int64_t cols,
                            double* __restrict__ dst, int64_t ld) {
  const int64_t r = blockIdx.y * (int64_t)blockDim.y + threadIdx.y, c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r < rows && c < cols) dst[r * ld + c] = src[r * sr + c * sc];
}

// The feature kernel: out[i][j] = amp cos(omega_j . (s o x_i) + phase_j) for a block of points, written into the left columns of
// the evaluation workspace (leading dimension ldo); rows i >= n and columns j >= nf of the tile grid are written as exact zeros.
// grid = (nfp / 64, np / 64), 256 threads, every thread 4 points x 4 features.  s o x and a tile of Omega are staged in LDS, PW_DC
// dimensions at a time, rows padded by one element (33 doubles: the 16 feature rows a wave reads start on 16 different bank pairs,
// the point row is a broadcast).  The dot product runs over d in ascending order whatever the block, so a point's features do not
// depend on where the point stands in the call.
__global__ __launch_bounds__(256) void k_pw_features(const double* __restrict__ x, int64_t ldx, int64_t n, int64_t D,
                                                     const double* __restrict__ scales, const double* __restrict__ omega,
                                                     const double* __restrict__ phase, int64_t nf, double amp,
                                                     double* __restrict__ out, int64_t ldo) {
  __shared__ double xs[64][PW_DC + 1];
  __shared__ double om[64][PW_DC + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)64, j0 = blockIdx.x * (int64_t)64;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int64_t d0 = 0; d0 < D; d0 += PW_DC) {
    const int dc = (int)((D - d0) < PW_DC ? (D - d0) : PW_DC);
    for (int e = tid; e < 64 * PW_DC; e += 256) {
      const int r = e / PW_DC, d = e % PW_DC;
      const int64_t i = i0 + r, j = j0 + r;
      xs[r][d] = (d < dc && i < n) ? scales[d0 + d] * x[i * ldx + d0 + d] : 0.0;
      om[r][d] = (d < dc && j < nf) ? omega[j * D + d0 + d] : 0.0;
    }
    __syncthreads();
    for (int d = 0; d < dc; ++d) {
      double xv[4], ov[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) xv[p] = xs[ty + 16 * p][d];
#pragma unroll
      for (int q = 0; q < 4; ++q) ov[q] = om[tx + 16 * q][d];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fma(xv[p], ov[q], acc[p][q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = j0 + tx + 16 * q;
    const double ph = j < nf ? phase[j] : 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int64_t i = i0 + ty + 16 * p;
      out[i * ldo + j] = (i < n && j < nf) ? amp * cos(acc[p][q] + ph) : 0.0;
    }
  }
}

// R[i][s] = U[i][s] + mu[i] - P[i][s] for i < m, s < S (in place in U, leading dimension ld): the residual u - Phi(Z) w of
// Matheron's rule, u = mu + Xa' e.  The padding keeps the zeros of its operands.
__global__ void k_pw_resid(int64_t m, int64_t S, int64_t ld, const double* __restrict__ mu, const double* __restrict__ P,
                           double* __restrict__ U) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y, s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < m && s < S) U[i * ld + s] = (U[i * ld + s] + mu[i]) - P[i * ld + s];
}
// exact GP: P[i][s] += sigma E[i][s] (the noisy prior draw at the training inputs)
__global__ void k_pw_add_noise(int64_t m, int64_t S, int64_t ld, double sigma, const double* __restrict__ E, double* __restrict__ P) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y, s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < m && s < S) P[i * ld + s] = P[i * ld + s] + sigma * E[i * ld + s];
}
// exact GP: V'[s][i] = alpha[i] - V'[s][i] for s < S, i < m (V' stored sample-major with leading dimension ld)
__global__ void k_pw_gp_finish(int64_t m, int64_t S, int64_t ld, const double* __restrict__ alpha, double* __restrict__ Vt) {
  const int64_t s = blockIdx.y * (int64_t)blockDim.y + threadIdx.y, i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < m && s < S) Vt[s * ld + i] = alpha[i] - Vt[s * ld + i];
}

}  // namespace agp
