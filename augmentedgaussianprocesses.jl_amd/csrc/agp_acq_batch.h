// Batch acquisition: the predictor conditioned on pending points at their own predicted mean (agp_svgp_acquisition_pending,
// agp_svgp_acq_maximize_batch; include/agp_hip.h "ACQUISITION FUNCTIONS", paragraph "Pending points").  Float64.
// The conditioned variance is the variance of an AUGMENTED predictor
//   Z' = [Z; P],  a' = [a; 0],  A' = [[A + V C^-1 V', -V C^-1], [-C^-1 V', C^-1]],  V = A K_ZP,   var_P(x) = (v + jitter) - k'(x)' A' k'(x)
// on which the contraction of agp_acq.h runs unchanged with m' = m + n.  A' is built by bordering, one point at a time in the order
// p_1, p_2, ...: with the current (Z', A') of size n' and the new point p stored as row n' of Z',
//   k' = k(Z', p),   w = A' k',   c = (v + jitter + tau2) - k'' w,   A'' = [[A' + w w'/c, -w/c], [-w'/c, 1/c]] = A' + u u'/c,  u = [w; -1]
// A' is NOT summed up: its entries reach 1 / c, and k'' A' k' would cancel to (v + jitter) - var_P with an absolute error of
// eps |A'| |k'|^2 -- with 63 points on one inducing point 1e-9 of the variance, which EI and PI magnify.  Kept are A0 = [[A, 0], [0, 0]]
// and the rank-one terms apart, U[b] = u_b and N[.][b] = -u_b / c_b, so that
//   A' k' = A0 k' - N (U k'),      W = K*m' A'^T = K*m' A0^T - (K*m' U^T) N^T      (three GEMMs per pass instead of one)
// and an error of g_b = u_b' k' enters k'' A' k' = k'' A0 k' + sum_b g_b^2 / c_b multiplied by g_b, which is small where c_b is.
//   k_acqb_kvec     k' : one thread per row of Z', q by direct differences in ascending d
//   k_acqb_matvec   A0 k' and U k' : one wave per row, lane l adds columns l, l + 64, ... ascending, then shuffles at 32, 16, ..., 1
//   k_acqb_wsum     w = A0 k' - N (U k') : one thread per row, the terms in ascending b
//   k_acqb_pivot    c : one workgroup, thread t adds j = t, t + 256, ..., then an LDS tree
//   k_acqb_store    row b of U and column b of N
// No atomics, nothing waits: every sum has an order fixed by n', and the launches follow one another on the stream.  c <= 0 or a
// non-finite c (impossible with jitter > 0 in exact arithmetic) is latched with a plain store in a word of the workspace's own
// that agp_svgp_check_status reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_cavi.h"  // kernel_base

namespace agp {

constexpr int ACQB_MAXPEND = 64;  // AGP_ACQ_MAX_PENDING: the augmented workspaces hold m + 64 points

// kv[j] = v phi(sum_d (s_d (z_jd - p_d))^2) for j < n, with p = row n of Z (rows dense, D wide).  variance < 0: the device-resident
// parameters (see k_kernelmatrix).
__global__ void k_acqb_kvec(const double* __restrict__ Z, int64_t n, int D, const double* __restrict__ scales, int kind, double variance,
                            double* __restrict__ kv) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double var = variance < 0.0 ? scales[D] : variance;
  const double* p = Z + n * D;
  const double* z = Z + j * D;
  double q = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = scales[d] * z[d] - scales[d] * p[d];
    q = __builtin_fma(t, t, q);
  }
  kv[j] = var * kernel_base<double>(kind, q);
}

// out[i] = sum_j A[i][j] kv[j] over j < cols, for i < rows: one wave per row, four rows per workgroup
__global__ void __launch_bounds__(256) k_acqb_matvec(const double* __restrict__ A, int64_t ld, int64_t rows, int64_t cols,
                                                     const double* __restrict__ kv, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  if (i >= rows) return;  // (the whole wave)
  const double* row = A + i * ld;
  double s = 0.0;
  for (int64_t j = lane; j < cols; j += 64) s = __builtin_fma(row[j], kv[j], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) out[i] = s;
}

// w[j] = w0[j] - sum_b N[j][b] g[b] over b < nb in ascending b, for j < n (N has ACQB_MAXPEND columns)
__global__ void k_acqb_wsum(int64_t n, int nb, const double* __restrict__ w0, const double* __restrict__ N, const double* __restrict__ g,
                            double* __restrict__ w) {
#pragma clang fp contract(off)
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = w0[j];
  for (int b = 0; b < nb; ++b) s = s - N[j * ACQB_MAXPEND + b] * g[b];
  w[j] = s;
}

// c[0] = kdiag - sum_j kv[j] w[j] over j < n (kdiag = v + jitter + tau2, formed on the host); one workgroup of 256 threads.  A c that
// is not a positive finite number sets *bad = 1 (nothing else ever writes 1 there; agp_svgp_check_status reads and clears it).
__global__ void __launch_bounds__(256) k_acqb_pivot(int64_t n, const double* __restrict__ kv, const double* __restrict__ w, double kdiag,
                                                    double* __restrict__ c, int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t j = tid; j < n; j += 256) s = __builtin_fma(kv[j], w[j], s);
  sh[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) sh[tid] = sh[tid] + sh[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double cv = kdiag - sh[0];
    c[0] = cv;
    if (!(cv > 0.0) || !(cv <= 1.79769313486231570815e308)) *bad = 1;
  }
}

// the new rank-one term u = [w; -1] over c: U[b][j] = w_j, U[b][n] = -1 and N[j][b] = -(w_j / c), N[n][b] = 1 / c for j < n, one
// thread per j <= n.  The caller guarantees n < ld and b < ACQB_MAXPEND; everything else of U and N keeps its zeros.
__global__ void k_acqb_store(int64_t n, int b, int64_t ld, const double* __restrict__ w, const double* __restrict__ c,
                             double* __restrict__ U, double* __restrict__ N) {
#pragma clang fp contract(off)
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j > n) return;
  const double cv = c[0];
  U[(int64_t)b * ld + j] = j < n ? w[j] : -1.0;
  N[j * ACQB_MAXPEND + b] = j < n ? -(w[j] / cv) : 1.0 / cv;
}

}  // namespace agp
