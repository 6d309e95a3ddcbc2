// Log predictive density (agp_svgp_lpd_stream / agp_log_predictive, include/agp_hip.h "LOG PREDICTIVE DENSITY"; DESIGN.md
// section 9m): the point-wise kernel that turns (mean_f, var_f, y) into lpd = log int p(y | f) N(f; mean_f, var_f) df, one partial
// sum per workgroup, and the fixed-order reduction over all partials.
//   Gaussian                 closed form  log N(y; mu, var + sigma2)
//   Laplace(beta)            closed form  (1 / 4 beta) [T(d) + T(-d)], T(d) = exp(var / 2 beta^2 - d / beta) erfc(a),
//                            a = (var / beta - d) / sqrt(2 var), d = y - mu; T is formed in logs (erfc below a = 0, erfcx above)
//   Logistic, BayesianSVM, StudentT, Poisson, NegBinomial
//                            log sum_j w_j p(y | mu + sqrt(var) x_j) over the caller's Gauss-Hermite rule (predictions.jl:4,
//                            classification.jl:14-26), as a log-sum-exp of log w_j + log p with every log p overflow-safe
//   LogisticSoftMax, SoftMax the link on the means (multiclass.jl:96-117): log sigma(mu_y) - log sum_k sigma(mu_k), resp.
//                            mu_y - logsumexp(mu)
// StudentT is the reference's density AS WRITTEN (studentt.jl:43-46): Gamma(alpha) / (sqrt(nu pi) Gamma(nu / 2)) (1 + ((y - f) /
// sigma)^2)^-alpha, alpha = (nu + 1) / 2 -- the normalised t with nu degrees of freedom and scale sigma / sqrt(nu), multiplied by
// sigma / sqrt(nu): the constant nvi_lconst uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_cavi.h"

namespace agp {

constexpr int LPD_THREADS = 256;
constexpr int LPD_GROUP = 16;  // lanes per point of the quadrature kinds (a DPP row)
constexpr unsigned long long LPD_NONE = ~0ull;  // "no such point" in the two failure words
constexpr int LIK_SOFTMAX = 10;                 // = AGP_LIK_SOFTMAX

// p0: Gaussian sigma2 / StudentT nu / Laplace beta / NegBinomial r / Poisson lambda (Gaussian and Poisson: overridden by the
// handle's state word when the kernel is given one); p1: StudentT sigma; c0: the part of log p that depends on neither f nor y,
// formed on the host (lgamma): StudentT's constant, -lgamma(r) for NegBinomial, -log(4 beta) for Laplace.
struct LpdParams {
  double p0, p1, c0;
};

__host__ __device__ constexpr bool lpd_is_quad(int kind) {
  return kind == LIK_LOGISTIC || kind == LIK_BSVM || kind == LIK_STUDENTT || kind == LIK_POISSON || kind == LIK_NEGBIN;
}
__host__ __device__ constexpr bool lpd_is_multiclass(int kind) { return kind == LIK_LSM || kind == LIK_SOFTMAX; }
__host__ __device__ constexpr int lpd_points_per_block(int kind) { return lpd_is_quad(kind) ? LPD_THREADS / LPD_GROUP : LPD_THREADS; }

// log sigma(x) = -log(1 + exp(-x)), overflow-safe on both sides (the z > 0 split of k_quad_local)
__device__ __forceinline__ double lpd_log_sigmoid(double x) { return x >= 0.0 ? -log1p(exp(-x)) : x - log1p(exp(x)); }
__device__ __forceinline__ double lpd_logaddexp(double a, double b) {
  const double M = fmax(a, b), d = -fabs(a - b);
  return d == d ? M + log1p(exp(d)) : M;  // (both -inf: a - b is NaN)
}
__device__ __forceinline__ bool lpd_finite(double x) { return fabs(x) < __builtin_inf(); }

// log T(d) of the Laplace closed form: below a = 0 erfc(a) is in (1, 2]; above, exp(var / 2 beta^2 - d / beta - a^2) = exp(-d^2 / 2 var)
// takes the growing exponential out and erfcx(a) stays in (0, 1]
__device__ __forceinline__ double lpd_laplace_logT(double d, double v, double s, double be) {
  const double a = (v / be - d) / (s * 1.4142135623730951);
  return a < 0.0 ? v / (2.0 * be * be) - d / be + log(erfc(a)) : -0.5 * d * d / v + log(erfcx(a));
}

// log Gamma(y + r) - log Gamma(y + 1), the part of NegBinomial's log C(y + r - 1, y) that depends on y.  Two lgammas of size y log y
// cancel to a value of size r log y (at y = 20000 one ulp of either is 3e-11): from y = 32 on the difference is formed from
// Stirling's series, lgamma(z) = (z - 1/2) log z - z + log(2 pi) / 2 + S(z), whose large parts are subtracted in closed form:
//   (y + 1/2) log1p((r - 1) / (y + 1)) + (r - 1) (log(y + r) - 1) + S(y + r) - S(y + 1);  the first omitted term of S is z^-9 / 1188.
__device__ __forceinline__ double lpd_stirling_tail(double z) {
  const double i = 1.0 / z, i2 = i * i;
  return i * (1.0 / 12.0 - i2 * (1.0 / 360.0 - i2 * (1.0 / 1260.0 - i2 * (1.0 / 1680.0))));
}
__device__ __forceinline__ double lpd_lgamma_diff(double y, double r) {
  if (y < 32.0) return lgamma(y + r) - lgamma(y + 1.0);
  return (y + 0.5) * log1p((r - 1.0) / (y + 1.0)) + (r - 1.0) * (log(y + r) - 1.0) + lpd_stirling_tail(y + r) -
         lpd_stirling_tail(y + 1.0);
}

// log p(y | f) + (what depends on y alone is in cy) of the quadrature kinds
template <int KIND>
__device__ __forceinline__ double lpd_logp(const LpdParams& P, double lam, double cy, double y, double f) {
  if constexpr (KIND == LIK_LOGISTIC) {
    return lpd_log_sigmoid(y * f);
  } else if constexpr (KIND == LIK_BSVM) {  // bayesiansvm.jl:25-38: pos / (pos + neg), pos = exp(-2 max(1 - y f, 0))
    const double z = y * f;
    return lpd_log_sigmoid(-2.0 * fmax(1.0 - z, 0.0) + 2.0 * fmax(1.0 + z, 0.0));
  } else if constexpr (KIND == LIK_STUDENTT) {
    const double u = (y - f) / P.p1;
    return P.c0 - 0.5 * (P.p0 + 1.0) * log1p(u * u);
  } else if constexpr (KIND == LIK_POISSON) {  // poisson.jl:26,34-36: Poisson(lambda sigma(f)); cy = y log lambda - lgamma(y + 1)
    const double ls = lpd_log_sigmoid(f);
    return cy + (y > 0.0 ? y * ls : 0.0) - lam * exp(ls);
  } else {  // NegBinomial(r, sigma(-f)), negativebinomial.jl:29,33-35; cy = lgamma(y + r) - lgamma(y + 1) - lgamma(r)
    return cy + P.p0 * lpd_log_sigmoid(-f) + (y > 0.0 ? y * lpd_log_sigmoid(f) : 0.0);
  }
}

// Points base .. base + nc of the stream; mu / var are the chunk's moments [nl][ld], y is read at the stream position (T[n], or
// int32 class indices for the multi-class kinds), lpd_out (nullable) is written there.
// Quadrature kinds: a 16-lane group per point (16 points per workgroup), node j on lane j mod 16, a running (max, scaled sum) pair
// per lane, the 16 pairs merged by a fixed xor-shuffle tree (8, 4, 2, 1): a 4096-point chunk is 256 workgroups.  The closed-form
// and multi-class kinds: one lane per point.  nodes[0 .. nn) | log weights[nn .. 2 nn).  Everything is accumulated in double.
// part[w] = block_sum of the workgroup's points, w = its index within the chunk (the caller offsets `part` by the chunk's first
// workgroup): no atomics on floating-point values.  bad[0] = smallest stream position whose var_f is not > 0 or whose moments are
// not finite; bad[1] = smallest stream position of a target the likelihood cannot take (class index outside [0, n_class), a count
// that is not a non-negative integer, a binary label that is not +-1).  Such a point adds nothing to the sum (the call fails).
// lstate (nullable): the handle's likelihood-state word (Gaussian noise under opt_noise, Poisson lambda), read instead of P.p0.
template <typename T, int KIND>
__global__ void __launch_bounds__(LPD_THREADS)
k_predict_lpd(int64_t nc, int64_t base, int nl, int64_t ld, LpdParams P, const T* __restrict__ lstate, const T* __restrict__ y,
              const int32_t* __restrict__ ycls, const T* __restrict__ mu, const T* __restrict__ var,
              const double* __restrict__ quad, int nn, T* __restrict__ lpd_out, double* __restrict__ part,
              unsigned long long* __restrict__ bad) {
  __shared__ double red[LPD_THREADS / 64];
  constexpr bool QUAD = lpd_is_quad(KIND);
  const int sub = QUAD ? (int)(threadIdx.x & (LPD_GROUP - 1)) : 0;
  const int64_t i = QUAD ? blockIdx.x * (int64_t)(LPD_THREADS / LPD_GROUP) + (threadIdx.x / LPD_GROUP)
                         : blockIdx.x * (int64_t)LPD_THREADS + threadIdx.x;
  double out = 0.0;
  bool have = false;
  if (i < nc) {
    const int64_t gi = base + i;
    bool ok = true;
    for (int k = 0; k < (lpd_is_multiclass(KIND) ? nl : 1); ++k) {
      const double mk = (double)mu[k * ld + i], vk = (double)var[k * ld + i];
      ok = ok && (vk > 0.0) && lpd_finite(mk) && lpd_finite(vk);
    }
    if (!ok) {
      if (sub == 0) atomicMin(&bad[0], (unsigned long long)gi);
    } else if constexpr (lpd_is_multiclass(KIND)) {
      const int cls = ycls[gi];
      if (cls < 0 || cls >= nl) {
        atomicMin(&bad[1], (unsigned long long)gi);
      } else {
        // log-sum-exp over the classes of log sigma(mu_k) (LogisticSoftMax) or mu_k (SoftMax), two passes
        double M = -__builtin_inf(), ly = 0.0;
        for (int k = 0; k < nl; ++k) {
          const double x = (double)mu[k * ld + i];
          const double l = KIND == LIK_LSM ? lpd_log_sigmoid(x) : x;
          M = fmax(M, l);
          if (k == cls) ly = l;
        }
        double s = 0.0;
        for (int k = 0; k < nl; ++k) {
          const double x = (double)mu[k * ld + i];
          s += exp((KIND == LIK_LSM ? lpd_log_sigmoid(x) : x) - M);
        }
        out = ly - (M + log(s));
        have = true;
      }
    } else {
      const double m = (double)mu[i], v = (double)var[i], yi = (double)y[gi];
      const double p0 = ((KIND == LIK_GAUSSIAN || KIND == LIK_POISSON) && lstate) ? (double)lstate[0] : P.p0;
      if constexpr (KIND == LIK_GAUSSIAN) {
        const double d = yi - m, vv = v + p0;
        out = -0.5 * (log(6.283185307179586 * vv) + d * d / vv);
        have = true;
      } else if constexpr (KIND == LIK_LAPLACE) {
        const double d = yi - m, s = sqrt(v);
        out = P.c0 + lpd_logaddexp(lpd_laplace_logT(d, v, s, p0), lpd_laplace_logT(-d, v, s, p0));
        have = true;
      } else {
        bool yok = true;
        if constexpr (KIND == LIK_LOGISTIC || KIND == LIK_BSVM) yok = (yi == 1.0 || yi == -1.0);
        if constexpr (KIND == LIK_POISSON || KIND == LIK_NEGBIN) yok = (yi >= 0.0) && lpd_finite(yi) && (floor(yi) == yi);
        if (!yok) {
          if (sub == 0) atomicMin(&bad[1], (unsigned long long)gi);
        } else {
          double cy = 0.0;
          if constexpr (KIND == LIK_POISSON) cy = yi * log(p0) - lgamma(yi + 1.0);
          if constexpr (KIND == LIK_NEGBIN) cy = lpd_lgamma_diff(yi, P.p0) + P.c0;
          const double s = sqrt(v);
          // running pair: sum_j exp(lw_j) = S exp(M) over this lane's nodes
          double M = -__builtin_inf(), S = 0.0;
          for (int j = sub; j < nn; j += LPD_GROUP) {
            const double lw = quad[nn + j] + lpd_logp<KIND>(P, p0, cy, yi, m + s * quad[j]);
            if (lw > -__builtin_inf()) {  // (a zero weight, or a density that is zero: nothing to add; NaN falls out too)
              const double e = exp(-fabs(lw - M));
              if (lw > M) {
                S = S * e + 1.0;
                M = lw;
              } else {
                S += e;
              }
            }
          }
          // the 16 pairs, merged in one fixed order; the merge is symmetric, so every lane of the group ends with the same bits
          for (int o = LPD_GROUP / 2; o > 0; o >>= 1) {
            const double M2 = __shfl_xor(M, o, LPD_GROUP), S2 = __shfl_xor(S, o, LPD_GROUP);
            if (M2 > -__builtin_inf()) {
              if (!(M > -__builtin_inf())) {
                M = M2;
                S = S2;
              } else {
                const double d = M - M2, e = exp(-fabs(d));
                S = d >= 0.0 ? S + S2 * e : S * e + S2;
                M = fmax(M, M2);
              }
            }
          }
          out = M + log(S);  // (no node with a positive density: -inf)
          have = sub == 0;
        }
      }
    }
    if (have && lpd_out) lpd_out[gi] = (T)out;
  }
  const double v = block_sum<double>(have ? out : 0.0, red);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// out[0] = the sum of part[w] over all nw workgroups of all chunks in ONE fixed order (thread t adds the partials t, t + 1024, ...
// in that order, then block_sum); out[1], out[2] = the two failure words as doubles (an index < 2^53), -1 = none.
__global__ void __launch_bounds__(1024)
k_lpd_reduce(const double* __restrict__ part, int64_t nw, const unsigned long long* __restrict__ bad, double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (int64_t w = threadIdx.x; w < nw; w += blockDim.x) s += part[w];
  s = block_sum<double>(s, red);
  if (threadIdx.x == 0) {
    out[0] = s;
    out[1] = bad[0] == LPD_NONE ? -1.0 : (double)bad[0];
    out[2] = bad[1] == LPD_NONE ? -1.0 : (double)bad[1];
  }
}

}  // namespace agp
