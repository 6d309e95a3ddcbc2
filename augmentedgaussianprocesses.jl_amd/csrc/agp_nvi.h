// agp_nvi.h -- numerical variational inference by Gauss-Hermite quadrature (QuadratureVI, src/inference/numericalVI.jl,
// src/inference/quadratureVI.jl): the point-wise expectations, the gradient assembly, the optimiser rules on (mu, Sigma) and the
// candidate Sigma + alpha Symmetric(dSigma) of the positive-definiteness backtracking.  The m x m products and the factorisation
// of the candidate are the library's own (gemm_nt, agp_blas_host.h; potrf_fused, agp_chol_host.h); the steps are Nvgp::nvi_step and
// Nsvgp::nvi_step (agp_capi.hip).
// At the end of the file: the expectations by Monte-Carlo integration over K latents (MCIntegrationVI, src/inference/MCVI.jl), which feed
// the same step once per latent.
// Three definitions of the reference are restated in their intended form (include/agp_hip.h, "NUMERICAL INFERENCE"):
//   Logistic  l'' = -sigma(f) sigma(-f)                       (logistic.jl:98-100 grows like exp(3 |f|))
//   Laplace   E[l''] = -(2 / beta) N(y; mu_f, var_f)          (laplace.jl:131 has the wrong sign and no exponential)
//   clipping  refused                                         (quadratureVI.jl:121-126 returns the opposite sign convention)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/agp_hip.h"  // AGP_LIK_*
#include "agp_cavi.h"

namespace agp {

enum { NVI_DESCENT = 1, NVI_MOMENTUM = 2, NVI_ADAM = 0 };  // = AGP_OPT_* (include/agp_hip.h)

// the optimiser rules of Optimisers.apply as the reference hands them the gradient (ascent: the caller ADDS the result)
//   Descent   d = eta g
//   Momentum  vel = rho vel + eta g ; d = vel                  (p1 = rho)
//   ADAM      m = b1 m + (1 - b1) g ; v = b2 v + (1 - b2) g^2 ; d = eta (m / c1) / (sqrt(v / c2) + eps),  c = 1 - b^t  (p1 = b1, p2 = b2)
struct NviRule {
  int kind;
  double eta, p1, p2, eps;
  double c1, c2;  // ADAM bias corrections 1 - b1^t, 1 - b2^t of THIS step (formed on the host)
};
__device__ __forceinline__ double nvi_rule(const NviRule& r, double g, double* __restrict__ s0, double* __restrict__ s1) {
  if (r.kind == NVI_DESCENT) return r.eta * g;
  if (r.kind == NVI_MOMENTUM) {
    const double vel = r.p1 * *s0 + r.eta * g;
    *s0 = vel;
    return vel;
  }
  const double mm = r.p1 * *s0 + (1.0 - r.p1) * g;
  const double vv = r.p2 * *s1 + (1.0 - r.p2) * g * g;
  *s0 = mm;
  *s1 = vv;
  return r.eta * (mm / r.c1) / (sqrt(vv / r.c2) + r.eps);
}

__device__ __forceinline__ double nvi_sigmoid(double x) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double e = exp(x);
  return e / (1.0 + e);
}

// One lane per point: ell = sum_j w_j l(y, f_j), g = sum_j w_j l'(y, f_j), h = sum_j w_j l''(y, f_j) at f_j = mu + sqrt(max(var, 0)) x_j
// (quadratureVI.jl:90-127; x_j = sqrt(2) t_j and w_j = omega_j / sqrt(pi) arrive ready-made, so the device and a host restatement
// share them bit for bit).  idx (nullable): the minibatch, y is read at idx[i].  lconst: the part of l that does not depend on f (formed on the host: lgamma).  Laplace: h in closed form.
template <typename T>
__global__ __launch_bounds__(256) void k_quad_local(int64_t n, LikParams<T> lp, double lconst, const T* __restrict__ y,
                                                     const int64_t* __restrict__ idx, const T* __restrict__ mu, const T* __restrict__ var,
                                                     const double* __restrict__ nodes, const double* __restrict__ weights, int nn,
                                                     T* __restrict__ ell, T* __restrict__ g, T* __restrict__ h) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double yi = (double)y[idx ? idx[i] : i], m = (double)mu[i], v = (double)var[i];
  const double sd = sqrt(v > 0.0 ? v : 0.0);
  double se = 0.0, sg = 0.0, sh = 0.0;
  if (lp.kind == AGP_LIK_LOGISTIC) {
    for (int j = 0; j < nn; ++j) {
      const double f = m + sd * nodes[j], w = weights[j];
      const double z = -yi * f;  // l = -log(1 + exp(-y f)), overflow-safe on both sides
      const double l = z > 0.0 ? -(z + log1p(exp(-z))) : -log1p(exp(z));
      se += w * l;
      sg += w * (yi * nvi_sigmoid(z));
      sh += w * (-nvi_sigmoid(f) * nvi_sigmoid(-f));
    }
  } else if (lp.kind == AGP_LIK_STUDENTT) {
    const double al = 0.5 * ((double)lp.p0 + 1.0), sig = (double)lp.p1;
    for (int j = 0; j < nn; ++j) {
      const double f = m + sd * nodes[j], w = weights[j];
      const double u = (yi - f) / sig, q = 1.0 + u * u;
      se += w * (lconst - al * log(q));
      sg += w * (2.0 * al * u / (sig * q));
      sh += w * (-2.0 * al * (1.0 - u * u) / (sig * sig * q * q));
    }
  } else {  // AGP_LIK_LAPLACE
    const double be = (double)lp.p0;
    for (int j = 0; j < nn; ++j) {
      const double f = m + sd * nodes[j], w = weights[j];
      const double d = yi - f;
      se += w * (lconst - fabs(d) / be);
      sg += w * ((d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)) / be);
    }
    const double d = yi - m;
    sh = v > 0.0 ? -(2.0 / be) * exp(-0.5 * d * d / v) / sqrt(6.283185307179586 * v) : 0.0;
  }
  ell[i] = (T)se;
  g[i] = (T)sg;
  h[i] = (T)sh;
}

// gradient of eta1 and the optimiser step on mu, one wave per row (numericalVI.jl:132,154,160-166):
//   natural    grad = K g - (mu - mu0)             (K (g - K^-1 (mu - mu0)); M = K)
//   classical  grad = g - K^-1 (mu - mu0)          (M = K^-1)
// d = rule(grad) goes to dmu; mu itself moves in k_nvi_add (every row reads all of mu here)
template <typename T>
__global__ __launch_bounds__(256) void k_nvi_grad_mu(int64_t m, int64_t ld, int natural, const T* __restrict__ M,
                                                      const T* __restrict__ g, const T* __restrict__ mu, const T* __restrict__ mu0,
                                                      NviRule rule, double* __restrict__ s0, double* __restrict__ s1,
                                                      T* __restrict__ dmu) {
  const int64_t row = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  double s = 0.0;
  for (int64_t k = lane; k < m; k += 64) {
    const double x = natural ? (double)g[k] : (double)mu[k] - (mu0 ? (double)mu0[k] : 0.0);
    s += (double)M[row * ld + k] * x;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) {
    const double grad = natural ? s - ((double)mu[row] - (mu0 ? (double)mu0[row] : 0.0)) : (double)g[row] - s;
    dmu[row] = (T)nvi_rule(rule, grad, s0 + row, s1 + row);
  }
}
template <typename T>
__global__ void k_nvi_add(int64_t m, T* __restrict__ mu, const T* __restrict__ dmu) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < m) mu[i] += dmu[i];
}

// A <- Sigma Diagonal(h) - A  (A = Sigma K^-1 on entry; h = NULL: A <- -A, the sparse model, whose data term is P2 of
// k_nvi_grad_sigma), the left factor of the natural gradient of eta2:
//   2 Sigma grad_eta2 Sigma = (Sigma Diagonal(h) - Sigma K^-1) Sigma + Sigma      -- no inverse of Sigma
template <typename T>
__global__ void k_nvi_left(int64_t m, int64_t n, int64_t ld, const T* __restrict__ Sigma, const T* __restrict__ h, T* __restrict__ A) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || j >= n) return;
  A[i * ld + j] = (i < m && j < m) ? (h ? Sigma[i * ld + j] * h[j] : T(0)) - A[i * ld + j] : T(0);
}

// gradient of eta2 on the upper triangle, the optimiser rule there, and D = Symmetric(dSigma) (upper triangle mirrored,
// numericalVI.jl:163-168); zero outside m x m.
//   natural    grad_ij = R_ij + Sigma_ij,  R = (Sigma Diagonal(h) - Sigma K^-1) Sigma           (P = R, Q unused)
//   classical  grad_ij = delta_ij h_i / 2 - (K^-1_ij - Sigma^-1_ij) / 2                         (P = K^-1, Q = Sigma^-1)
// Sparse model (P2 given, h not read): natural grad = P + Sigma + P2 with P = -Sigma K^-1 Sigma, P2 = rho W Diagonal(h) W', W = Sigma kappa';
// classical grad = P2 / 2 - (K^-1 - Sigma^-1) / 2 with P2 = rho kappa' Diagonal(h) kappa.
// The optimiser state of the strict lower triangle is never read by the reference's update (Symmetric reads the upper one): it
// stays zero here.
template <typename T>
__global__ void k_nvi_grad_sigma(int64_t m, int64_t n, int64_t ld, int natural, const T* __restrict__ P, const T* __restrict__ Q,
                                 const T* __restrict__ P2, const T* __restrict__ Sigma, const T* __restrict__ h, NviRule rule, double* __restrict__ s0,
                                 double* __restrict__ s1, T* __restrict__ Dm) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || j >= n) return;
  if (i >= m || j >= m) {
    Dm[i * ld + j] = T(0);
    return;
  }
  if (i > j) return;  // written by (j, i)
  const int64_t e = i * ld + j;
  double grad;
  if (natural)
    grad = (double)P[e] + (double)Sigma[e] + (P2 ? (double)P2[e] : 0.0);
  else
    grad = (P2 ? 0.5 * (double)P2[e] : (i == j ? 0.5 * (double)h[i] : 0.0)) - 0.5 * ((double)P[e] - (double)Q[e]);
  const double d = nvi_rule(rule, grad, s0 + e, s1 + e);
  Dm[e] = (T)d;
  Dm[j * ld + i] = (T)d;
}

// C = Sigma + alpha D inside m x m, the identity in the padding; F = a second copy, which the factorisation overwrites
template <typename T>
__global__ void k_nvi_candidate(int64_t m, int64_t n, int64_t ld, const T* __restrict__ Sigma, const T* __restrict__ Dm, T alpha,
                                T* __restrict__ C, T* __restrict__ F) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || j >= n) return;
  const T v = (i < m && j < m) ? Sigma[i * ld + j] + alpha * Dm[i * ld + j] : (i == j ? T(1) : T(0));
  if (C) C[i * ld + j] = v;
  F[i * ld + j] = v;
}

// ---- sparse model: the minibatch moments and the kappa-weighted pieces of the gradient -----------------------------------------------
// One wave per minibatch point i: K~_i = k_ii + jitt - kappa_i . Knm_i, mean_f,i = kappa_i . mu, var_f,i = kappa_i . W_.i + K~_i with
// Wt = Sigma kappa' (m x B, leading dimension ldw)      latentgp.jl:171-189, 209-212
template <typename T>
__global__ __launch_bounds__(256) void k_nvi_fstats(int64_t B, int64_t m, int64_t ldk, int64_t ldw, const T* __restrict__ kappa,
                                                     const T* __restrict__ Knm, const T* __restrict__ Wt, const T* __restrict__ mu,
                                                     T kdiag, T* __restrict__ mf, T* __restrict__ vf) {
  const int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= B) return;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int64_t k = lane; k < m; k += 64) {
    const double kp = (double)kappa[i * ldk + k];
    a += kp * (double)Knm[i * ldk + k];
    b += kp * (double)mu[k];
    c += kp * (double)Wt[k * ldw + i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
    c += __shfl_down(c, o);
  }
  if (lane == 0) {
    mf[i] = (T)b;
    vf[i] = (T)(c + ((double)kdiag - a));
  }
}
// out = S Diagonal(rho w) over the B valid columns (zero beyond), S m x B with leading dimension ld, n x nq stored
template <typename T>
__global__ void k_nvi_scale_cols(int64_t m, int64_t B, int64_t n, int64_t nq, int64_t ld, const T* __restrict__ S, const T* __restrict__ w,
                                 T rho, T* __restrict__ out) {
  const int64_t i = blockIdx.y * (int64_t)blockDim.y + threadIdx.y;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || j >= nq) return;
  out[i * ld + j] = (i < m && j < B) ? S[i * ld + j] * (rho * w[j]) : T(0);
}
// u = rho kappa' g: one wave per row of kappa' (m x B, leading dimension ld); zero in the padding rows
template <typename T>
__global__ __launch_bounds__(256) void k_nvi_kappat_g(int64_t m, int64_t n, int64_t B, int64_t ld, const T* __restrict__ kapt,
                                                       const T* __restrict__ g, T rho, T* __restrict__ u) {
  const int64_t row = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  double s = 0.0;
  if (row < m)
    for (int64_t k = lane; k < B; k += 64) s += (double)kapt[row * ld + k] * (double)g[k];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) u[row] = (T)((double)rho * s);
}

// ---- MC integration (MCIntegrationVI, src/inference/MCVI.jl; include/agp_hip.h, "MC INTEGRATION") ------------------------------------
// ell_i = mean_s log p(c_i | f_s), g_ik = mean_s d log p / d f_k, h_ik = mean_s d2 log p / d f_k^2 at f_sk = mu_ik + sqrt(max(var_ik, 0)) eps_sk
// for the SoftMax and the LogisticSoftMax likelihood (softmax.jl:26-48, logisticsoftmax.jl:144-193), from the nMC x K table eps of the
// step (k_mc_normals).  One wave per point, four points per workgroup.  The lanes of a wave are (draw, latent) pairs: with P the power
// of two >= K, lane = grp P + k handles latent k of draw s0 + grp, 64 / P draws at a time, so the maximum and the sums over k are P-lane
// butterflies and every lane owns ONE accumulator of g_k and of h_k -- no per-lane array over k.  The table is staged through LDS in
// tiles of MC_TILE doubles (whole draws), shared by the four waves.  Summation order: a lane adds its draws in order, then a fixed
// butterfly over the groups; it depends on (nMC, K) alone, never on the grid.
// 1 - s_k of the largest entry is formed as (sum of the other entries) / total (the first maximum counts as the largest), which keeps
// the relative accuracy of g_c and h_k where a class probability approaches one.
// idx (nullable): the minibatch, the class is read at idx[i].  mu, var: [K][ldp]; g, h: [K][ldo].  flags (nullable): FLAG_BAD_LABEL.
constexpr int MC_TILE = 2048;
constexpr int MC_KMAX = 64;
__global__ __launch_bounds__(256) void k_mc_local(int64_t n, int lik, int K, int nMC, const int32_t* __restrict__ ycls,
                                                   const int64_t* __restrict__ idx, const double* __restrict__ mu,
                                                   const double* __restrict__ var, int64_t ldp, const double* __restrict__ eps,
                                                   double* __restrict__ ell, double* __restrict__ g, double* __restrict__ h, int64_t ldo,
                                                   int* __restrict__ flags) {
  __shared__ double tile[MC_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = blockIdx.x * (int64_t)4 + wave;
  const bool active = i < n;  // (wave-uniform; an idle wave still loads its share of the tile and meets the barriers)
  int P = 2;
  while (P < K) P <<= 1;
  const int G = 64 / P, grp = lane / P, k = lane & (P - 1);
  const bool valid = k < K;
  const unsigned long long gmask = P == 64 ? ~0ull : ((1ull << P) - 1ull);
  int cls = -1;
  double m = 0.0, sd = 0.0;
  if (active) {
    cls = ycls[idx ? idx[i] : i];
    if ((cls < 0 || cls >= K) && flags && lane == 0) atomicOr(flags, FLAG_BAD_LABEL);
    if (valid) {
      const double v = var[k * ldp + i];
      m = mu[k * ldp + i];
      sd = sqrt(v > 0.0 ? v : 0.0);
    }
  }
  const bool mine = valid && k == cls;
  const int TS = MC_TILE / K;  // draws per tile (K <= MC_KMAX: at least 32)
  double ae = 0.0, ag = 0.0, ah = 0.0;
  for (int t0 = 0; t0 < nMC; t0 += TS) {
    const int ns = nMC - t0 < TS ? nMC - t0 : TS;
    __syncthreads();
    for (int e = threadIdx.x; e < ns * K; e += 256) tile[e] = eps[(int64_t)t0 * K + e];
    __syncthreads();
    if (!active) continue;
    for (int s0 = 0; s0 < ns; s0 += G) {  // (uniform over the wave: every lane takes part in the butterflies)
      const int s = s0 + grp;
      const bool on = valid && s < ns;
      const double f = on ? m + sd * tile[s * K + k] : -__builtin_inf();
      double M = f;
      for (int o = P >> 1; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o));
      const unsigned long long tops = (__ballot(on && f == M) >> (grp * P)) & gmask;
      const bool top = on && k == __ffsll((long long)tops) - 1;
      if (lik == AGP_LIK_SOFTMAX) {
        const double e = on ? exp(f - M) : 0.0;  // (the largest: exactly 1)
        double Sp = top ? 0.0 : e;
        for (int o = P >> 1; o > 0; o >>= 1) Sp += __shfl_xor(Sp, o);
        const double S = 1.0 + Sp, sk = e / S, om = top ? Sp / S : 1.0 - sk;
        if (on) {
          ag += mine ? om : -sk;
          ah += -sk * om;
          if (mine) ae += (f - M) - log1p(Sp);
        }
      } else {  // AGP_LIK_LOGISTICSOFTMAX
        const double ex = exp(-fabs(f)), den = 1.0 + ex;
        const double sg = on ? (f >= 0.0 ? 1.0 / den : ex / den) : 0.0;   // logistic(f)
        const double sm = f >= 0.0 ? ex / den : 1.0 / den;                // 1 - logistic(f) = logistic(-f)
        double Sp = top ? 0.0 : sg, St = top ? sg : 0.0;
        for (int o = P >> 1; o > 0; o >>= 1) {
          Sp += __shfl_xor(Sp, o);
          St += __shfl_xor(St, o);
        }
        const double S = St + Sp, sk = sg / S, om = top ? Sp / S : 1.0 - sk;
        if (on) {
          const double d = mine ? om : -sk;  // y_k - s_k
          ag += sm * d;
          ah += sm * (-sg * d - sk * om * sm);
          // log s_c: of the largest entry -log1p(others / sg_c) (no cancellation where s_c approaches one), else log sg_c - log S
          // with log sg_c = -softplus(-f_c)
          if (mine) ae += top ? -log1p(Sp / sg) : (f >= 0.0 ? -log1p(ex) : f - log1p(ex)) - log(S);
        }
      }
    }
  }
  if (!active) return;
  for (int o = 32; o > 0; o >>= 1) ae += __shfl_xor(ae, o);
  for (int o = 32; o >= P; o >>= 1) {  // over the groups: the lanes that hold the same latent
    ag += __shfl_xor(ag, o);
    ah += __shfl_xor(ah, o);
  }
  if (lane == 0) ell[i] = ae / (double)nMC;
  if (grp == 0 && valid) {
    g[k * ldo + i] = ag / (double)nMC;
    h[k * ldo + i] = ah / (double)nMC;
  }
}

// SoftMax link on the means only (multiclass.jl:96-117, softmax.jl): out[i][k] row-major n x nl, two passes over k
template <typename T>
__global__ void k_proba_softmax(int64_t n, int nl, int64_t ldm, const T* __restrict__ mu, T* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double M = (double)mu[i];
  for (int k = 1; k < nl; ++k) M = fmax(M, (double)mu[k * ldm + i]);
  double s = 0.0;
  for (int k = 0; k < nl; ++k) s += exp((double)mu[k * ldm + i] - M);
  for (int k = 0; k < nl; ++k) out[i * nl + k] = (T)(exp((double)mu[k * ldm + i] - M) / s);
}

}  // namespace agp
