// agp_greedy.h -- kernel-aware inducing-point selection on the device: greedy conditional-variance selection, the algorithm behind
// `inducingpoints(ConditionalVariance(m, kernel), X)`.  It is the greedy MAP of a k-DPP (Chen, Zhang, Zhou 2018) and the greedy
// variance selection of Burt, Rasmussen, van der Wilk (2020): a pivoted partial Cholesky factorisation of K_NN that takes, at every
// step, the point with the largest remaining conditional variance given the points already chosen.  What it reduces greedily,
// tr(K_NN - K_NZ K_ZZ^-1 K_ZN), is the trace term of the SVGP ELBO.
//
//   d_i = k(x_i, x_i) = variance ; for j = 0 .. m-1:
//     p_j = argmax_i d_i (ties -> smaller i) ; stop if d_{p_j} <= tol * variance
//     l_j = (k(X, x_{p_j}) - sum_{k<j} l_k l_k[p_j]) / sqrt(d_{p_j}) ; d <- d - l_j^2 ; d_{p_j} <- 0 (never chosen again)
//
// Float64 throughout.  Two launches per step, nothing travels to the host between them:
//   k_gv_step   : one lane per point.  Kernel value against the pivot's coordinates (squared distance in ascending d, kernel_base of
//                 agp_cavi.h), minus the row-dot with the j previous columns -- the pivot's j coefficients are staged through LDS in
//                 chunks of GV_CHUNK and read as broadcasts; four interleaved accumulators, column k into accumulator k & 3 -- then the
//                 lane's entry of column j, its new d_i, and a per-workgroup (max, argmax, sum d) partial.
//   k_gv_finish : one workgroup.  Reduces the partials (every thread a contiguous range in workgroup order, then a fixed tree), writes
//                 the residual trace, the next pivot, its coordinates (also the row of z_out, a bit copy) and its coefficient row, or
//                 the stop flag.  After a stop both kernels return at once.
// The factor is kept column-contiguous, F[m][Np] (Np = N padded to the workgroup), so that step j streams j coalesced columns; the
// points are read from a one-off transposed Float64 copy Xt[D][Np].  Workgroups are 256 points whatever the size, partials are combined
// in a fixed order and there are no floating-point atomics: the result is a function of the inputs alone.
#pragma once
#include "agp_cavi.h"  // kernel_base
#include "agp_device.h"

namespace agp {

constexpr int GV_MAXD = 128;   // the k-means limit
constexpr int GV_BLOCK = 256;  // points per workgroup, one per lane
constexpr int GV_CHUNK = 256;  // pivot coefficients staged per LDS pass (a multiple of 4: the accumulator of column k is k & 3)

struct GvPart {
  double vmax;
  int64_t imax;
  double sum;
};
struct GvState {
  int64_t p;     // current pivot
  double dp;     // its residual variance d_p
  int32_t stop;  // the residual fell to tol * variance: every later launch is a no-op
  int32_t nsel;  // points chosen so far
};

__device__ __forceinline__ void gv_better(double& v, int64_t& i, double v2, int64_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// (max, argmax with ties to the smaller index, sum) over the workgroup; the result is valid in every thread.  red: 4 entries.
__device__ __forceinline__ GvPart gv_block_reduce(double v, int64_t i, double s, GvPart* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_down(v, o);
    const long long i2 = __shfl_down((long long)i, o);
    s += __shfl_down(s, o);
    gv_better(v, i, v2, (int64_t)i2);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    red[wave].vmax = v;
    red[wave].imax = i;
    red[wave].sum = s;
  }
  __syncthreads();
  GvPart r = red[0];
#pragma unroll
  for (int w = 1; w < GV_BLOCK / 64; ++w) {
    gv_better(r.vmax, r.imax, red[w].vmax, red[w].imax);
    r.sum += red[w].sum;
  }
  return r;
}

// out[c * ldout + r] = (double)in[r * ldin + c] for r < rows, c < cols, in 32 x 32 tiles through LDS; a linear grid of
// ceil(rows / 32) * ceil(cols / 32) workgroups of 32 x 8 threads.  Xt from X, and factor_out from the column-contiguous factor.
template <typename Tin>
__global__ __launch_bounds__(256) void k_gv_transpose(const Tin* __restrict__ in, int64_t ldin, int64_t rows, int64_t cols,
                                                      double* __restrict__ out, int64_t ldout) {
  __shared__ double t[32][33];
  const int64_t tiles_c = (cols + 31) / 32;
  const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * 32, c0 = ((int64_t)blockIdx.x % tiles_c) * 32;
  for (int q = threadIdx.y; q < 32; q += 8) {
    const int64_t r = r0 + q, c = c0 + threadIdx.x;
    if (r < rows && c < cols) t[q][threadIdx.x] = (double)in[r * ldin + c];
  }
  __syncthreads();
  for (int q = threadIdx.y; q < 32; q += 8) {
    const int64_t c = c0 + q, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[c * ldout + r] = t[threadIdx.x][q];
  }
}

// d_i = k(x_i, x_i) = variance, and the partials the first k_gv_finish picks p_0 = 0 from
__global__ __launch_bounds__(GV_BLOCK) void k_gv_init(int64_t N, double variance, double* __restrict__ dres,
                                                      GvPart* __restrict__ part) {
  __shared__ GvPart red[GV_BLOCK / 64];
  const int64_t i = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  const bool live = i < N;
  if (live) dres[i] = variance;
  const GvPart r = gv_block_reduce(live ? variance : -INFINITY, live ? i : INT64_MAX, live ? variance : 0.0, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(GV_BLOCK) void k_gv_step(const double* __restrict__ Xt, const double* __restrict__ scales, int64_t N,
                                                      int64_t Np, int D, int kind, double variance, int64_t j,
                                                      double* __restrict__ F, double* __restrict__ dres,
                                                      const GvState* __restrict__ st, const double* __restrict__ zp,
                                                      const double* __restrict__ lp, GvPart* __restrict__ part) {
  __shared__ double coef[GV_CHUNK];
  __shared__ double zs[GV_MAXD], ss[GV_MAXD];
  __shared__ GvPart red[GV_BLOCK / 64];
  if (st->stop) return;
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * GV_BLOCK + tid;
  const bool live = i < N;
  const int64_t p = st->p;
  const double dp = st->dp;
  if (tid < D) {
    zs[tid] = zp[tid];
    ss[tid] = scales[tid];
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t k0 = 0; k0 < j; k0 += GV_CHUNK) {
    const int nk = (int)(j - k0 < GV_CHUNK ? j - k0 : GV_CHUNK);
    __syncthreads();  // the previous chunk is consumed
    if (tid < nk) coef[tid] = lp[k0 + tid];
    __syncthreads();
    if (live) {
      const double* col = F + k0 * Np + i;
      int kk = 0;
#pragma unroll 2
      for (; kk + 4 <= nk; kk += 4) {
        const double f0 = col[(int64_t)kk * Np], f1 = col[(int64_t)(kk + 1) * Np], f2 = col[(int64_t)(kk + 2) * Np],
                     f3 = col[(int64_t)(kk + 3) * Np];
        a0 += f0 * coef[kk];
        a1 += f1 * coef[kk + 1];
        a2 += f2 * coef[kk + 2];
        a3 += f3 * coef[kk + 3];
      }
      if (kk < nk) a0 += col[(int64_t)kk * Np] * coef[kk];
      if (kk + 1 < nk) a1 += col[(int64_t)(kk + 1) * Np] * coef[kk + 1];
      if (kk + 2 < nk) a2 += col[(int64_t)(kk + 2) * Np] * coef[kk + 2];
    }
  }
  __syncthreads();  // zs / ss (and the only barrier of step 0)
  double dnew = -INFINITY;
  if (live) {
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double t = ss[d] * (Xt[(int64_t)d * Np + i] - zs[d]);
      d2 += t * t;
    }
    const double c = variance * kernel_base<double>(kind, d2);
    const double l = (c - ((a0 + a1) + (a2 + a3))) / sqrt(dp);
    F[j * Np + i] = l;
    dnew = i == p ? 0.0 : dres[i] - l * l;
    dres[i] = dnew;
  }
  const GvPart r = gv_block_reduce(dnew, live ? i : INT64_MAX, live ? dnew : 0.0, red);
  if (tid == 0) part[blockIdx.x] = r;
}

// After step j (j = -1: after k_gv_init): the trace after j + 1 points, and pivot j + 1 or the stop flag.
template <typename T>
__global__ __launch_bounds__(GV_BLOCK) void k_gv_finish(const GvPart* __restrict__ part, int64_t nblk, int64_t j, int64_t m, double thr,
                                                        const T* __restrict__ X, int64_t ldx, int D, const double* __restrict__ F,
                                                        int64_t Np, GvState* __restrict__ st, double* __restrict__ zp,
                                                        double* __restrict__ lp, int64_t* __restrict__ idx_out,
                                                        T* __restrict__ z_out, int64_t ldz, double* __restrict__ trace_out) {
  __shared__ GvPart red[GV_BLOCK / 64];
  if (st->stop) return;  // (read by every thread before the barriers of the reduction, written behind them)
  const int tid = threadIdx.x;
  const int64_t per = (nblk + GV_BLOCK - 1) / GV_BLOCK;
  const int64_t b0 = tid * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  double v = -INFINITY, s = 0.0;
  int64_t ix = INT64_MAX;
  for (int64_t b = b0; b < b1; ++b) {
    gv_better(v, ix, part[b].vmax, part[b].imax);
    s += part[b].sum;
  }
  const GvPart r = gv_block_reduce(v, ix, s, red);
  if (tid == 0 && j >= 0 && trace_out) trace_out[j] = r.sum;
  if (j + 1 >= m) return;
  if (!(r.vmax > thr)) {
    if (tid == 0) st->stop = 1;
    return;
  }
  const int64_t p = r.imax;
  if (tid == 0) {
    st->p = p;
    st->dp = r.vmax;
    st->nsel = (int32_t)(j + 2);
    idx_out[j + 1] = p;
  }
  for (int d = tid; d < D; d += GV_BLOCK) {
    const T xv = X[p * ldx + d];
    zp[d] = (double)xv;
    z_out[(j + 1) * ldz + d] = xv;
  }
  for (int64_t k = tid; k <= j; k += GV_BLOCK) lp[k] = F[k * Np + p];
}

// idx_out = -1 and z_out = 0 in exactly m (x D) elements, whatever ldz
template <typename T>
__global__ void k_gv_prefill(int64_t m, int D, int64_t* __restrict__ idx_out, T* __restrict__ z_out, int64_t ldz,
                             double* __restrict__ trace_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < m) {
    idx_out[e] = -1;
    if (trace_out) trace_out[e] = 0.0;
  }
  if (e < m * D) z_out[(e / D) * ldz + e % D] = T(0);
}

}  // namespace agp
