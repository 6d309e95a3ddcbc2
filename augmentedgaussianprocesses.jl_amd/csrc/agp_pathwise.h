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

// ---- multi-start ascent of the paths (agp_pathwise_maximize; include/agp_hip.h "PATHWISE SAMPLING") -----------------------------------
// A particle is a pair (sample s, start r), number s R + r.  k_pw_ascent runs the whole T-step ADAM ascent of a tile of PT particles
// in one workgroup and one launch: particles never need each other, so there is no communication between workgroups.  Per step the
// features (j < l) and then the inducing points (r < m) pass through LDS in tiles of 64 rows:
//   phase 1  thread (tx, ty) forms, for its particles p = ty + 16 pp and its rows j = tx + 16 q, a_pj = omega_j' (s o x_p) or q_pr =
//            sum_d (s_d x_pd - s_d Z_rd)^2 over d ascending, and writes B_pj = -amp sin(a_pj + p_j) W_j,s(p) or 2 variance phi'(q_pr)
//            V_r,s(p) into LDS (exact zeros for rows past l or m)
//   phase 2  thread (tx, ty) owns the coordinates d = tx + 16 q of the same particles, with x, the ADAM moments and the gradient sum
//            in registers, and adds sum_j B_pj omega_jd or sum_r B_pr (s_d x_pd - s_d Z_rd) over the tile's 64 rows in ascending order
// so every sum of a particle runs over j, then r, ascending, in one accumulator, whatever the tile it stands in: the same bits
// wherever it stands in the call.  After step T one more pass with cos and phi in place of -sin and 2 phi' sums the rows of B into
// f_s(x), again in ascending order.  No atomics, no scratch.  PT: 16 particles per tile fill 256 CUs with 4096 particles; larger
// tiles re-use a staged tile of Omega or Z more often but leave CUs idle (DESIGN.md section 9k has the measurement).
constexpr int PW_AD = 64;  // the largest D of the ascent: x, m, v and g of a tile live in registers next to the staging
struct PwAscentBox {       // by value in the kernel's arguments: nothing is copied, nothing synchronises
  double lo[PW_AD], hi[PW_AD], lr[PW_AD];
};

template <int PT, int DQ>
__global__ __launch_bounds__(256) void k_pw_ascent(const double* __restrict__ x0, int64_t ldx0, int x0_shared, int64_t R, int64_t np,
                                                   int64_t D, const double* __restrict__ scales, const double* __restrict__ omega,
                                                   const double* __restrict__ phase, int64_t nf, double amp,
                                                   const double* __restrict__ Z, int64_t m, int kind, double variance,
                                                   const double* __restrict__ WV, int64_t ldw, int64_t Lp, int steps, double sign,
                                                   double beta1, double beta2, double eps, const PwAscentBox box,
                                                   double* __restrict__ Xw, double* __restrict__ Fw) {
#pragma clang fp contract(off)
  constexpr int PP = PT / 16, DW = 16 * DQ;
  __shared__ double xs[PT][DW + 1];  // s o x of the tile's particles
  __shared__ double tl[64][DW + 1];  // 64 rows of Omega, or of s o Z
  __shared__ double Bs[PT][64 + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t p0 = blockIdx.x * (int64_t)PT;
  int64_t wrow[PP];  // the particle's row of [W' | V']; a tile's surplus particles repeat the call's last one and are not stored
  double x[PP][DQ], mo[PP][DQ], vo[PP][DQ], sd[DQ], lo[DQ], hi[DQ], lr[DQ];
#pragma unroll
  for (int q = 0; q < DQ; ++q) {
    const int d = tx + 16 * q;
    const bool in = d < D;
    sd[q] = in ? scales[d] : 0.0, lo[q] = in ? box.lo[d] : 0.0, hi[q] = in ? box.hi[d] : 0.0, lr[q] = in ? box.lr[d] : 0.0;
  }
#pragma unroll
  for (int pp = 0; pp < PP; ++pp) {
    const int64_t pi = (p0 + ty + 16 * pp) < np ? (p0 + ty + 16 * pp) : np - 1;
    wrow[pp] = (pi / R) * ldw;
    const double* xr = x0 + (x0_shared ? pi % R : pi) * ldx0;
#pragma unroll
    for (int q = 0; q < DQ; ++q) {
      const int d = tx + 16 * q;
      x[pp][q] = d < D ? fmin(fmax(xr[d], lo[q]), hi[q]) : 0.0;
      mo[pp][q] = vo[pp][q] = 0.0;
      xs[ty + 16 * pp][d] = sd[q] * x[pp][q];
    }
  }
  double b1k = 1.0, b2k = 1.0, fsum = 0.0;
  for (int k = 0; k <= steps; ++k) {
    const bool fin = k == steps;  // the pass after the last step: the values at the final x
    double g[PP][DQ], xsd[PP][DQ];
#pragma unroll
    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
      for (int q = 0; q < DQ; ++q) g[pp][q] = 0.0, xsd[pp][q] = sd[q] * x[pp][q];
    for (int part = 0; part < 2; ++part) {  // the features, then the inducing points
      const int64_t n = part ? m : nf, col0 = part ? Lp : 0;
      for (int64_t j0 = 0; j0 < n; j0 += 64) {
        for (int e = tid; e < 64 * DW; e += 256) {
          const int r = e / DW, d = e % DW;
          const int64_t j = j0 + r;
          tl[r][d] = (d < D && j < n) ? (part ? scales[d] * Z[j * D + d] : omega[j * D + d]) : 0.0;
        }
        __syncthreads();  // the tile, and s o x of the step before
        double acc[PP][4];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[pp][q] = 0.0;
        for (int d = 0; d < (int)D; ++d) {
          double xv[PP], tv[4];
#pragma unroll
          for (int pp = 0; pp < PP; ++pp) xv[pp] = xs[ty + 16 * pp][d];
#pragma unroll
          for (int q = 0; q < 4; ++q) tv[q] = tl[tx + 16 * q][d];
#pragma unroll
          for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (part) {
                const double t = xv[pp] - tv[q];
                acc[pp][q] = fma(t, t, acc[pp][q]);
              } else {
                acc[pp][q] = fma(xv[pp], tv[q], acc[pp][q]);
              }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t j = j0 + tx + 16 * q;
          const bool in = j < n;
          const double ph = (in && !part) ? phase[j] : 0.0;
#pragma unroll
          for (int pp = 0; pp < PP; ++pp) {
            double b = 0.0;
            if (in) {
              if (part) b = fin ? variance * kernel_base<double>(kind, acc[pp][q]) : (2.0 * variance) * kernel_dbase<double>(kind, acc[pp][q]);
              else b = fin ? amp * cos(acc[pp][q] + ph) : -amp * sin(acc[pp][q] + ph);
              b *= WV[wrow[pp] + col0 + j];
            }
            Bs[ty + 16 * pp][tx + 16 * q] = b;
          }
        }
        __syncthreads();
        if (fin) {
          if (tid < PT)
            for (int jj = 0; jj < 64; ++jj) fsum += Bs[tid][jj];
        } else {
          for (int jj = 0; jj < 64; ++jj) {
            double bv[PP], tv[DQ];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) bv[pp] = Bs[ty + 16 * pp][jj];
#pragma unroll
            for (int q = 0; q < DQ; ++q) tv[q] = tl[jj][tx + 16 * q];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp)
#pragma unroll
              for (int q = 0; q < DQ; ++q) g[pp][q] = fma(bv[pp], part ? xsd[pp][q] - tv[q] : tv[q], g[pp][q]);
          }
        }
        __syncthreads();  // before the next tile overwrites tl and Bs
      }
    }
    if (fin) break;
    b1k *= beta1, b2k *= beta2;
    const double c1 = 1.0 - b1k, c2 = 1.0 - b2k;
#pragma unroll
    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
      for (int q = 0; q < DQ; ++q) {
        const double gr = sign * (sd[q] * g[pp][q]);
        mo[pp][q] = beta1 * mo[pp][q] + (1.0 - beta1) * gr;
        vo[pp][q] = beta2 * vo[pp][q] + (1.0 - beta2) * (gr * gr);
        const double xn = x[pp][q] + lr[q] * ((mo[pp][q] / c1) / (sqrt(vo[pp][q] / c2) + eps));
        x[pp][q] = fmin(fmax(xn, lo[q]), hi[q]);
        xs[ty + 16 * pp][tx + 16 * q] = sd[q] * x[pp][q];  // read behind the next tile's barrier
      }
  }
#pragma unroll
  for (int pp = 0; pp < PP; ++pp) {
    const int64_t pi = p0 + ty + 16 * pp;
#pragma unroll
    for (int q = 0; q < DQ; ++q)
      if (pi < np && tx + 16 * q < D) Xw[pi * D + tx + 16 * q] = x[pp][q];
  }
  if (tid < PT && p0 + tid < np) Fw[p0 + tid] = fsum;
}

// The reduction over the starts of one sample (one workgroup per sample): the start with the largest sign f, ties to the smallest r;
// a NaN never wins, and if every value is NaN start 0 does.  Comparisons only, so the order of the scan does not matter.  Writes the
// best value, its index and the x of that start; each output may be NULL.
__global__ __launch_bounds__(256) void k_pw_ascent_best(const double* __restrict__ Xw, const double* __restrict__ Fw, int64_t R, int64_t D,
                                                        double sign, double* __restrict__ best_x, int64_t ldb,
                                                        double* __restrict__ best_f, int64_t* __restrict__ best_idx) {
  __shared__ double sv[256];
  __shared__ int64_t si[256];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const double* F = Fw + s * R;
  double bv = 0.0;
  int64_t bi = -1;  // -1: nothing but NaN so far
  for (int64_t r = tid; r < R; r += 256) {
    const double v = sign * F[r];
    if (v == v && (bi < 0 || v > bv)) bv = v, bi = r;
  }
  sv[tid] = bv, si[tid] = bi;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const double ov = sv[tid + h];
      const int64_t oi = si[tid + h];
      if (oi >= 0 && (si[tid] < 0 || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) sv[tid] = ov, si[tid] = oi;
    }
    __syncthreads();
  }
  const int64_t b = si[0] < 0 ? 0 : si[0];
  if (tid == 0) {
    if (best_f) best_f[s] = F[b];
    if (best_idx) best_idx[s] = b;
  }
  if (best_x)
    for (int d = tid; d < D; d += 256) best_x[s * ldb + d] = Xw[(s * R + b) * D + d];
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
