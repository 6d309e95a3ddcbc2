// agp_pathwise.h -- device code of pathwise (decoupled) posterior sampling (Wilson et al. 2020; include/agp_hip.h, "PATHWISE
// SAMPLING"): the spectral draw of the random Fourier features, the Normal tables W and E, the feature kernel Phi(x) and the small
// element-wise kernels of the draw, and the kernels of the paths' input gradients (agp_pathwise_eval_grad: k_pw_dkern,
// k_pw_grad_operand, k_pw_grad_scatter).  The products of the draw, of an evaluation and of a gradient are the library's own (gemm_nt,
// k_gemm_tn).
// Every table entry is a function of (seed, t, stream, index) alone -- streams 4 + 8 l .. 8 + 8 l of latent l -- with log and
// cos 2 pi by the arithmetic of streams 2 and 3 (agp_rand.h), so a host program reproduces Omega, the phases, W and E bit for bit
// (tests/_pathwise_ref.py does).  No kernel here uses scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_hyper.h"  // kernel_dbase
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
// depend on where the point stands in the call.  SIN: out[i][j] = -amp sin(...), the derivative of the feature with respect to its
// argument (the A block of the gradient's base workspace), by the same staging and the same sum.
template <bool SIN>
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
      if (SIN) out[i * ldo + j] = (i < n && j < nf) ? -amp * sin(acc[p][q] + ph) : 0.0;
      else out[i * ldo + j] = (i < n && j < nf) ? amp * cos(acc[p][q] + ph) : 0.0;
    }
  }
}

// ---- input gradients of the paths (agp_pathwise_eval_grad; include/agp_hip.h "PATHWISE SAMPLING") -------------------------------------
// With t_ird = s_d (x_id - Z_rd), q_ir = sum_d t_ird^2 and c_ir = variance phi'(q_ir) (kernel_dbase: finite at r = 0, no division by r)
//   d f_s / d x_d (x_i) = s_d sum_j A_ij omega_jd W_js + 2 s_d sum_r c_ir t_ird V_rs ,   A_ij = -amp sin(omega_j' (s o x_i) + p_j)
// formed per dimension d as one gemm_nt of Wd = [A_ij s_d omega_jd | 2 s_d c_ir t_ird] against the stored [W' | V'] -- the call of the
// evaluation -- from the base workspace B0 = [A | C] that is written once per chunk (k_pw_features<true>, k_pw_dkern).
constexpr int PW_GD = 64;  // dimensions whose slabs are staged together before they are transposed into the caller's [s][i][d] rows

// C[i][r] = variance phi'(q_ir) for a block of points against a block of Z, the right columns of the base workspace; rows i >= n and
// columns r >= m of the tile grid are exact zeros.  grid = (mp / 64, np / 64), 256 threads, 4 points x 4 inducing points per thread,
// the LDS staging of k_pw_features (rows of 33 doubles).  q is summed over d in ascending order from direct differences of the scaled
// coordinates: no GEMM-form cancellation far from the origin, and a point's row does not depend on where it stands in the call.
__global__ __launch_bounds__(256) void k_pw_dkern(const double* __restrict__ x, int64_t ldx, int64_t n, int64_t D,
                                                  const double* __restrict__ scales, const double* __restrict__ Z, int64_t m, int kind,
                                                  double variance, double* __restrict__ out, int64_t ldo) {
  __shared__ double xs[64][PW_DC + 1];
  __shared__ double zs[64][PW_DC + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)64, r0 = blockIdx.x * (int64_t)64;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int64_t d0 = 0; d0 < D; d0 += PW_DC) {
    const int dc = (int)((D - d0) < PW_DC ? (D - d0) : PW_DC);
    for (int e = tid; e < 64 * PW_DC; e += 256) {
      const int r = e / PW_DC, d = e % PW_DC;
      const int64_t i = i0 + r, j = r0 + r;
      xs[r][d] = (d < dc && i < n) ? scales[d0 + d] * x[i * ldx + d0 + d] : 0.0;
      zs[r][d] = (d < dc && j < m) ? scales[d0 + d] * Z[j * D + d0 + d] : 0.0;
    }
    __syncthreads();
    for (int d = 0; d < dc; ++d) {
      double xv[4], zv[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) xv[p] = xs[ty + 16 * p][d];
#pragma unroll
      for (int q = 0; q < 4; ++q) zv[q] = zs[tx + 16 * q][d];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = xv[p] - zv[q];
          acc[p][q] = fma(t, t, acc[p][q]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t r = r0 + tx + 16 * q;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int64_t i = i0 + ty + 16 * p;
      out[i * ldo + r] = (i < n && r < m) ? variance * kernel_dbase<double>(kind, acc[p][q]) : 0.0;
    }
  }
}

// The operand of dimension d: Wd[i][j] = A_ij s_d omega_jd for j < Lp and Wd[i][Lp + r] = 2 s_d C_ir t_ird for r < mp, t_ird = s_d x_id -
// s_d Z_rd (0 exactly where x_i = Z_r), over the nq x (Lp + mp) workspace with leading dimension ld; one lane per element, consecutive
// lanes along a row.  The padding of B0 is zero and stays zero: nothing is read for rows >= n, features >= nf or inducing points >= m.
__global__ __launch_bounds__(256) void k_pw_grad_operand(const double* __restrict__ B0, int64_t nq, int64_t n, int64_t Lp, int64_t nf,
                                                         int64_t mp, int64_t m, int64_t ld, const double* __restrict__ x, int64_t ldx,
                                                         int64_t D, int64_t d, const double* __restrict__ scales,
                                                         const double* __restrict__ omega, const double* __restrict__ Z,
                                                         double* __restrict__ Wd) {
  const int64_t w = Lp + mp, e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= nq * w) return;
  const int64_t i = e / w, c = e - i * w;
  double v = 0.0;
  if (i < n) {
    const double sd = scales[d];
    if (c < Lp) {
      if (c < nf) v = B0[i * ld + c] * (sd * omega[c * D + d]);
    } else if (c - Lp < m) {
      const double t = sd * x[i * ldx + d] - sd * Z[(c - Lp) * D + d];
      v = (2.0 * sd) * (B0[i * ld + c] * t);
    }
  }
  Wd[i * ld + c] = v;
}

// The transposing scatter: G[k][s][i] (the slabs of dimensions d0 + k, k < nd <= PW_GD; slab stride lds_, row stride ldc) into the
// caller's out[s][i][d0 + k] at out + (s los + i) ldg + d0 + k, s < S, i < n.  grid = (S, ceil(n / 64)): a block reads 64 points of
// its sample from every slab along i, turns them in LDS (rows padded by one double: the transposed read walks 32 distinct bank pairs
// per half wave) and writes, per point, the run of nd consecutive doubles.
__global__ __launch_bounds__(256) void k_pw_grad_scatter(const double* __restrict__ G, int64_t lds_, int64_t ldc, int64_t n, int nd,
                                                         double* __restrict__ out, int64_t los, int64_t ldg, int64_t d0) {
  __shared__ double tile[PW_GD][64 + 1];
  const int tid = threadIdx.x;
  const int64_t i0 = blockIdx.y * (int64_t)64, s = blockIdx.x;
  const int ni = (int)((n - i0) < 64 ? (n - i0) : 64);
  for (int e = tid; e < nd * 64; e += 256) {
    const int k = e >> 6, i = e & 63;
    if (i < ni) tile[k][i] = G[k * lds_ + s * ldc + i0 + i];
  }
  __syncthreads();
  double* o = out + (s * los + i0) * ldg + d0;
  for (int e = tid; e < ni * nd; e += 256) {
    const int i = e / nd, k = e - i * nd;
    o[(int64_t)i * ldg + k] = tile[k][i];
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
