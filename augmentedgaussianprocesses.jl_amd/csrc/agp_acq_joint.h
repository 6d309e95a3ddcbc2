// Joint Monte-Carlo batch acquisition (q-EI, q-UCB) of q' = q + n points under their posterior correlation (agp_svgp_acquisition_joint,
// agp_svgp_acq_maximize_joint; include/agp_hip.h "ACQUISITION FUNCTIONS", paragraph "Joint batches").  Float64.
//   mu_j = k*(x_j)' a      C_jl = k(x_j, x_l) - k*(x_j)' A k*(x_l) + jitter [j == l]      C = L L'      f_s = mu + L eps_s
//   q-EI  alpha = (1/S) sum_s max(0, max_j (s (f_sj - best) - xi))        q-UCB  alpha = (1/S) sum_s max_j (s mu_j + beta sqrt(pi/2) |(L eps_s)_j|)
// Per step and chunk of sets, after K*m and W = K*m A' of the chunk's q points per set (the predictor's two launches):
//   k_acqj_cov      mu and the lower triangle of C of a set from its rows of K*m and W (and those of the pending points, formed once
//                   per call): one wave per column of the triangle, lanes strided over m, a butterfly at the end
//   k_acqj_set      C = L L' in LDS, the S samples with their maximum and the winner's index, alpha, and the backward pass: mu-bar,
//                   L-bar by a sum over the samples in a fixed order, Phi = tril(L' L-bar) with the diagonal halved,
//                   C-bar = sym(L^-T Phi L^-1)
//   k_acqj_weights  V_j = mu-bar_j a - 2 sum_l C-bar_jl W_l (the weight row of member j, which k_acq_contract's W channel contracts
//                   against dk/dx) and the point-to-point term 2 sum_l C-bar_jl d1 k(x_j, x_l)
//   k_acqj_step     the gather over the column groups, the clipping and the ADAM recurrence of k_acq_step
// The q' x q' objects live in LDS, a sample's base draws in fully unrolled registers.  No atomics: every sum has an order fixed by
// (m, D, q', S), and a workgroup sees one set only, so a set's result does not depend on its neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_acq.h"

namespace agp {

constexpr int AJ_Q = 16;                  // AGP_ACQ_JOINT_MAX_Q: q + n_pending
constexpr int AJ_LD = AJ_Q + 1;           // the pitch of a q' x q' matrix in LDS
constexpr int AJ_SMAX = 4096;             // samples
constexpr int AJ_THREADS = 256;           // = AJ_Q * AJ_Q: one thread per entry
constexpr int AJ_REC = AJ_Q * AJ_Q + AJ_Q;  // a set's record: [16][16] (C, then C-bar) and [16] (mu, then mu-bar)

// row j of a set's K*m or W: an optimised member (j < q) stands in the chunk's matrix, a pending one in the call's
__device__ __forceinline__ const double* aj_row(int j, int q, int64_t r, const double* __restrict__ M, const double* __restrict__ Mp,
                                                int64_t ld) {
  return j < q ? M + (r * q + j) * ld : Mp + (int64_t)(j - q) * ld;
}
__device__ __forceinline__ const double* aj_point(int j, int q, int64_t r, const double* __restrict__ X, int64_t ldx,
                                                  const double* __restrict__ P, int64_t ldp) {
  return j < q ? X + (r * q + j) * ldx : P + (int64_t)(j - q) * ldp;
}
__device__ __forceinline__ double aj_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// task t of a lower triangle stored row after row: (j, l), l <= j
__device__ __forceinline__ void aj_pair(int t, int& j, int& l) {
  j = 0;
  while (t > j) t -= j + 1, ++j;
  l = t;
}

// One workgroup per set r: rec[r] = (the lower triangle of C, mu).  A task is a column l of the triangle: mu_l = sum_i K_li a_i and, for
// every j >= l, C_jl = k(x_j, x_l) - sum_i W_ji K_li, the diagonal (v + jitter) - sum_i W_li K_li as the predictor forms its variance.
// A wave takes the columns l = w, w + 4, ...; a lane reads K_li for i = lane, lane + 64, ... once, in ascending order, and feeds the
// q' - l + 1 sums (unrolled registers); a butterfly adds the lanes.  pend (nullable): the record of the pending points among
// themselves (this kernel with q = 0), copied instead of being formed again.
__global__ void __launch_bounds__(AJ_THREADS)
k_acqj_cov(int q, int n, const double* __restrict__ X, int64_t ldx, const double* __restrict__ P, int64_t ldp,
           const double* __restrict__ K, const double* __restrict__ W, const double* __restrict__ Kp, const double* __restrict__ Wp,
           int64_t ld, int64_t m, const double* __restrict__ a, int D, const double* __restrict__ scales, int kind, double variance,
           double kdiag_jit, const double* __restrict__ pend, double* __restrict__ rec) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, qp = q + n;
  const int64_t r = blockIdx.x;
  const double var = variance < 0.0 ? scales[D] : variance;
  double* out = rec + r * AJ_REC;
  for (int l = w; l < qp; l += 4) {
    if (pend && l >= q) {  // (j >= l: the whole column is pending)
      if (lane == 0) out[AJ_Q * AJ_Q + l] = pend[AJ_Q * AJ_Q + (l - q)];
      if (lane >= l && lane < qp) out[lane * AJ_Q + l] = pend[(lane - q) * AJ_Q + (l - q)];
      continue;
    }
    const double* kl = aj_row(l, q, r, K, Kp, ld);
    const double* wr[AJ_Q];
#pragma unroll
    for (int j = 0; j < AJ_Q; ++j) wr[j] = aj_row(j < qp ? j : l, q, r, W, Wp, ld);
    double acc[AJ_Q], am = 0.0;
#pragma unroll
    for (int j = 0; j < AJ_Q; ++j) acc[j] = 0.0;
    for (int64_t i = lane; i < m; i += 64) {
      const double kv = kl[i];
      am = __builtin_fma(a[i], kv, am);
#pragma unroll
      for (int j = 0; j < AJ_Q; ++j)
        if (j >= l && j < qp) acc[j] = __builtin_fma(wr[j][i], kv, acc[j]);
    }
    am = aj_wave_sum(am);
    if (lane == 0) out[AJ_Q * AJ_Q + l] = am;
    const double* xl = aj_point(l, q, r, X, ldx, P, ldp);
    const double sd = lane < D ? scales[lane] : 0.0, xls = lane < D ? xl[lane] * sd : 0.0;
#pragma unroll
    for (int j = 0; j < AJ_Q; ++j) {
      if (j >= l && j < qp) {
        const double u = aj_wave_sum(acc[j]);
        double kjl = kdiag_jit;
        if (j != l) {
          const double* xj = aj_point(j, q, r, X, ldx, P, ldp);
          double t2 = 0.0;
          if (lane < D) {
            const double d = xj[lane] * sd - xls;
            t2 = d * d;
          }
          t2 = aj_wave_sum(t2);
          double kb, kd;
          kernel_base_dbase<double>(kind, t2, kb, kd);
          kjl = var * kb;
        }
        if (lane == 0) out[j * AJ_Q + l] = kjl - u;
      }
    }
  }
}

// One workgroup per set, thread (j, l) = (tid / 16, tid % 16) per matrix entry.  In: rec[r] = (C, mu).  Out: alpha[r] and, with
// grad != 0, bar[r] = (C-bar, full and symmetric, zero beyond q'; mu-bar).
//   1. C = L L' right-looking, the entry in a register, L in LDS; a pivot that is not positive and finite sets *bad (every writer
//      stores the same 1) and the set's results are NaN
//   2. thread t takes the samples s = t, t + 256, ...: eps_s in registers, z_j = sum_{k <= j} L_jk eps_sk in ascending k, the value of
//      each member in ascending j, the first maximum wins; win[s] (255: the sample does not count) and coef[s] go to LDS, the sample's
//      term to the thread's sum; the 256 sums are added by a tree through LDS
//   3. L-bar_jk = (1/S) sum_s [win_s == j] coef_s eps_sk and the counts of mu-bar: the q'(q'+1)/2 + q' tasks times as many slices of
//      the samples as fit in 256 threads, a slice in ascending s, the slices in ascending order
//   4. Phi = tril(L' L-bar), diagonal halved; L^-1 by right-looking forward substitution; C-bar = sym(L^-T (Phi L^-1))
__global__ void __launch_bounds__(AJ_THREADS, 2)
k_acqj_set(AcqParams p, int qp, int S, const double* __restrict__ eps, int64_t lde, const double* __restrict__ rec, int grad,
           double* __restrict__ alpha, double* __restrict__ bar, int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ double Ls[AJ_Q * AJ_LD], Lb[AJ_Q * AJ_LD], Ph[AJ_Q * AJ_LD], Li[AJ_Q * AJ_LD], Tm[AJ_Q * AJ_LD];
  __shared__ double mus[AJ_Q], cnt[AJ_Q], red[AJ_THREADS], coef[AJ_SMAX];
  __shared__ unsigned char win[AJ_SMAX];
  const int tid = threadIdx.x, j = tid >> 4, l = tid & 15;
  const int64_t r = blockIdx.x;
  const double* in = rec + r * AJ_REC;
  const bool low = j < qp && l <= j;
  double c = low ? in[j * AJ_Q + l] : 0.0;
  Ls[j * AJ_LD + l] = 0.0;
  Li[j * AJ_LD + l] = 0.0;
  Lb[j * AJ_LD + l] = 0.0;
  if (tid < AJ_Q) mus[tid] = tid < qp ? in[AJ_Q * AJ_Q + tid] : 0.0;
  __syncthreads();
  for (int k = 0; k < qp; ++k) {
    if (j == k && l == k) {
      if (!(c > 0.0) || !(c <= 1.79769313486231570815e308)) *bad = 1;
      Ls[k * AJ_LD + k] = sqrt(c);
    }
    __syncthreads();
    if (low && l == k && j > k) Ls[j * AJ_LD + k] = c / Ls[k * AJ_LD + k];
    __syncthreads();
    if (low && l > k) c = __builtin_fma(-Ls[j * AJ_LD + k], Ls[l * AJ_LD + k], c);
  }
  // the samples
  const bool ei = p.kind == 1;
  const double bc = p.beta * 1.25331413731550025121;  // sqrt(pi / 2)
  double asum = 0.0;
  for (int s = tid; s < S; s += AJ_THREADS) {
    __asm__ volatile("" ::: "memory");  // L is read from LDS per sample: hoisted, its 136 entries would cost half the occupancy
    double e[AJ_Q];
#pragma unroll
    for (int k = 0; k < AJ_Q; ++k) e[k] = k < qp ? eps[(int64_t)s * lde + k] : 0.0;
    double bv = 0.0, bz = 0.0;
    int bj = 0;
#pragma unroll
    for (int jj = 0; jj < AJ_Q; ++jj) {
      if (jj < qp) {
        double z = 0.0;
#pragma unroll
        for (int k = 0; k <= jj; ++k) z = __builtin_fma(Ls[jj * AJ_LD + k], e[k], z);
        const double val = ei ? p.s * ((mus[jj] + z) - p.best) - p.xi : p.s * mus[jj] + bc * fabs(z);
        if (jj == 0 || val > bv) bv = val, bj = jj, bz = z;
      }
    }
    if (ei) {
      const bool counts = bv > 0.0;
      asum += counts ? bv : (bv != bv ? bv : 0.0);
      win[s] = counts ? (unsigned char)bj : (unsigned char)255;
      coef[s] = p.s;
    } else {
      asum += bv;
      win[s] = (unsigned char)bj;
      coef[s] = bz > 0.0 ? bc : (bz < 0.0 ? -bc : 0.0);
    }
  }
  red[tid] = asum;
  __syncthreads();
  for (int h = AJ_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) alpha[r] = red[0] / (double)S;
  if (!grad) return;
  __syncthreads();  // (red is reused)
  // L-bar and the counts
  const int npair = qp * (qp + 1) / 2, ntask = npair + qp;
  int nsl = AJ_THREADS / ntask;
  if (nsl > S) nsl = S;
  const int len = (S + nsl - 1) / nsl;
  const int task = tid % ntask, sl = tid / ntask;
  int tj = 0, tk = 0;
  const bool is_cnt = task >= npair;
  if (is_cnt) tj = task - npair;
  else aj_pair(task, tj, tk);
  if (sl < nsl) {
    const int s0 = sl * len, s1 = s0 + len < S ? s0 + len : S;
    double acc = 0.0;
#pragma unroll 4
    for (int s = s0; s < s1; ++s) {  // (the loads do not wait for the winner: they are in flight together)
      const double ev = eps[(int64_t)s * lde + tk], cf = coef[s];
      if (win[s] == tj) acc = is_cnt ? acc + 1.0 : __builtin_fma(cf, ev, acc);
    }
    red[sl * ntask + task] = acc;
  }
  __syncthreads();
  if (tid < ntask) {
    double acc = 0.0;
    for (int v = 0; v < nsl; ++v) acc += red[v * ntask + task];
    if (is_cnt) cnt[tj] = p.s * acc / (double)S;
    else Lb[tj * AJ_LD + tk] = acc / (double)S;
  }
  __syncthreads();
  {  // Phi
    double ph = 0.0;
    if (low) {
#pragma unroll
      for (int k = 0; k < AJ_Q; ++k) ph = __builtin_fma(Ls[k * AJ_LD + j], Lb[k * AJ_LD + l], ph);
      if (j == l) ph *= 0.5;
    }
    Ph[j * AJ_LD + l] = ph;
  }
  // L^-1: L X = I, the entry (j, l) of X in a register until row j is final
  double x = (j == l && j < qp) ? 1.0 : 0.0;
  for (int k = 0; k < qp; ++k) {
    if (j == k) Li[k * AJ_LD + l] = x / Ls[k * AJ_LD + k];
    __syncthreads();
    if (j > k && j < qp) x = __builtin_fma(-Ls[j * AJ_LD + k], Li[k * AJ_LD + l], x);
  }
  __syncthreads();  // (Ph too)
  {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < AJ_Q; ++k) t = __builtin_fma(Ph[j * AJ_LD + k], Li[k * AJ_LD + l], t);
    Tm[j * AJ_LD + l] = t;
  }
  __syncthreads();
  {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < AJ_Q; ++k) t = __builtin_fma(Li[k * AJ_LD + j], Tm[k * AJ_LD + l], t);
    Ph[j * AJ_LD + l] = t;  // (the last reads of Ph stand before the barrier above)
  }
  __syncthreads();
  double* out = bar + r * AJ_REC;
  out[j * AJ_Q + l] = 0.5 * (Ph[j * AJ_LD + l] + Ph[l * AJ_LD + j]);
  if (tid < AJ_Q) out[AJ_Q * AJ_Q + tid] = tid < qp ? cnt[tid] : 0.0;
}

// Grid (ceil(m / 256), sets).  Thread i of a workgroup: the column i of the q weight rows of set r,
//   V[(r q + j)][i] = mu-bar_j a_i - 2 sum_{l < q'} C-bar_jl W_l[i]      (l ascending; W_l in registers, C-bar in LDS)
// and the workgroups with blockIdx.x == 0 the point-to-point term of the set,
//   cross[(r q + j)][d] = 2 sum_{l != j} C-bar_jl d k(x_j, x_l) / d x_jd = 4 s_d sum_l C-bar_jl c_jl t_jld,   c = v phi'(|t|^2), t = s (x_j - x_l)
// with the scaled points staged in LDS and one thread per pair for c.
__global__ void __launch_bounds__(AJ_THREADS)
k_acqj_weights(int q, int n, const double* __restrict__ X, int64_t ldx, const double* __restrict__ P, int64_t ldp,
               const double* __restrict__ W, const double* __restrict__ Wp, int64_t ld, int64_t m, const double* __restrict__ a, int D,
               const double* __restrict__ scales, int kind, double variance, const double* __restrict__ bar, double* __restrict__ V,
               int64_t ldv, double* __restrict__ cross) {
#pragma clang fp contract(off)
  __shared__ double cb[AJ_Q * AJ_LD], mb[AJ_Q], xs[AJ_Q * PG_MAXD], cc[AJ_Q * AJ_LD];
  const int tid = threadIdx.x, qp = q + n;
  const int64_t r = blockIdx.y;
  const double* in = bar + r * AJ_REC;
  cb[(tid >> 4) * AJ_LD + (tid & 15)] = in[tid];
  if (tid < AJ_Q) mb[tid] = in[AJ_Q * AJ_Q + tid];
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)AJ_THREADS + tid;
  if (i < m) {
    double w[AJ_Q];
#pragma unroll
    for (int l = 0; l < AJ_Q; ++l) w[l] = l < qp ? aj_row(l, q, r, W, Wp, ld)[i] : 0.0;
    const double ai = a[i];
#pragma unroll
    for (int j = 0; j < AJ_Q; ++j) {
      if (j < q) {
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < AJ_Q; ++l)
          if (l < qp) acc = __builtin_fma(cb[j * AJ_LD + l], w[l], acc);
        V[(r * q + j) * ldv + i] = mb[j] * ai - 2.0 * acc;
      }
    }
  }
  if (blockIdx.x != 0) return;
  const double var = variance < 0.0 ? scales[D] : variance;
  for (int e = tid; e < qp * D; e += AJ_THREADS) {
    const int l = e / D, d = e % D;
    xs[e] = aj_point(l, q, r, X, ldx, P, ldp)[d] * scales[d];
  }
  __syncthreads();
  {
    const int j = tid >> 4, l = tid & 15;
    double v = 0.0;
    if (j < q && l < qp && l != j) {
      double t2 = 0.0;
      for (int d = 0; d < D; ++d) {
        const double t = xs[j * D + d] - xs[l * D + d];
        t2 = __builtin_fma(t, t, t2);
      }
      double kb, kd;
      kernel_base_dbase<double>(kind, t2, kb, kd);
      v = cb[j * AJ_LD + l] * (var * kd);
    }
    cc[j * AJ_LD + l] = v;
  }
  __syncthreads();
  for (int e = tid; e < q * D; e += AJ_THREADS) {
    const int j = e / D, d = e % D;
    double acc = 0.0;
    for (int l = 0; l < qp; ++l) acc = __builtin_fma(cc[j * AJ_LD + l], xs[j * D + d] - xs[l * D + d], acc);
    cross[(r * q + j) * D + d] = 4.0 * scales[d] * acc;
  }
}

// d alpha / d x_id of particle i (member i % q of set i / q): the groups of k_acq_contract's W channel, which ran on the weight rows V,
// in ascending order, times 2 s_d, plus the point-to-point term
__device__ __forceinline__ double aj_grad(int64_t i, int d, int D, int ng, const double* __restrict__ part,
                                          const double* __restrict__ cross, const double* __restrict__ scales) {
#pragma clang fp contract(off)
  double gv = 0.0;
  for (int g = 0; g < ng; ++g) gv += part[(((int64_t)PG_MAXGROUPS + g) * PG_CH + i) * D + d];
  return 2.0 * scales[d] * gv + cross[i * D + d];
}

// agp_svgp_acquisition_joint: grad_out of a chunk of particles, one thread per (i, d)
__global__ void k_acqj_grad(int64_t np, int D, int ng, const double* __restrict__ part, const double* __restrict__ cross,
                            const double* __restrict__ scales, double* __restrict__ grad, int64_t ldg) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= np * D) return;
  const int64_t i = e / D;
  const int d = (int)(e % D);
  grad[i * ldg + d] = aj_grad(i, d, D, ng, part, cross, scales);
}

// One ADAM step of k_acq_step's recurrence on the particles of a chunk of sets, one thread per (i, d)
__global__ void k_acqj_step(int64_t np, int D, int ng, const double* __restrict__ part, const double* __restrict__ cross,
                            const double* __restrict__ scales, double beta1, double beta2, double c1, double c2, double eps,
                            const PwAscentBox box, double* __restrict__ x, double* __restrict__ mo, double* __restrict__ vo) {
#pragma clang fp contract(off)
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= np * D) return;
  const int64_t i = e / D;
  const int d = (int)(e % D);
  const double gr = aj_grad(i, d, D, ng, part, cross, scales);
  const double m1 = beta1 * mo[e] + (1.0 - beta1) * gr;
  const double v1 = beta2 * vo[e] + (1.0 - beta2) * (gr * gr);
  mo[e] = m1;
  vo[e] = v1;
  const double xn = x[e] + box.lr[d] * ((m1 / c1) / (sqrt(v1 / c2) + eps));
  x[e] = fmin(fmax(xn, box.lo[d]), box.hi[d]);
}

}  // namespace agp
