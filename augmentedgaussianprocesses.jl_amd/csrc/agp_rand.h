// agp_rand.h -- random variates on the device: the counter-based generator, the samplers of the augmentation variables and the two
// kernels of a Gibbs sweep of the full model (MCGP(X, y, kernel, likelihood, GibbsSampling()), src/models/MCGP.jl,
// src/inference/gibbssampling.jl).  Everything a draw depends on is (seed, sweep t, stream id, point i): no state is carried from
// launch to launch, so a draw does not depend on the grid, on the order in which waves run, or on how a chain is split over calls.
// The bit layout, the stream ids and the order in which a sampler consumes its uniforms are the contract of include/agp_hip.h
// ("random streams"): a host program that follows it reproduces a chain (tests/_mcgp_ref.py does).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_cavi.h"

namespace agp {

enum {  // next to FLAG_NEG_KTILDE / FLAG_BAD_LABEL
  FLAG_RNG_BOUND = 4,  // a sampler's loop ran into its iteration bound
  FLAG_BAD_COUNT = 8   // a NegBinomial target that is no non-negative integer (PG(y + r, c) needs an integer y + r >= 1)
};
enum { RNG_STREAM_LOCAL = 0, RNG_STREAM_NORMAL = 1 };
constexpr int RNG_LOOP_MAX = 1000;      // every rejection loop (acceptance >= ~0.5 per round: never reached by a correct sampler)
constexpr int RNG_SERIES_MAX = 64;      // terms of the alternating series a(n, x) (observed: decided at n = 1)
constexpr int64_t RNG_PG_B_MAX = 65536;  // PG(b, c) as a sum of b draws: the largest b = y + r

// Philox4x32-10 (Salmon et al. 2011; Random123): ctr = (c0, c1, c2, c3), key = (k0, k1)
struct Philox4 {
  uint32_t w[4];
};
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// two words -> one double in (0, 1): k = the top 27 bits of hi, then the top 26 of lo; u = (k + 0.5) 2^-53
__host__ __device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  const uint64_t k = ((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6);
  return ((double)k + 0.5) * 0x1.0p-53;
}

// the sequence u_0, u_1, ... of one (seed, t, stream, i): u_2j, u_2j+1 come from block j = Philox(ctr = (i, t, stream, j), key = seed)
struct RngStream {
  uint32_t i, t, stream, j, k0, k1;
  double held;
  int have;
  int* flags;
  __device__ __forceinline__ RngStream(uint64_t seed, uint32_t t_, uint32_t stream_, uint32_t i_, int* flags_)
      : i(i_), t(t_), stream(stream_), j(0), k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), held(0.0), have(0), flags(flags_) {}
  __device__ __forceinline__ double u() {
    if (have) {
      have = 0;
      return held;
    }
    const Philox4 b = philox4x32_10(i, t, stream, j, k0, k1);
    j += 1;
    held = u53(b.w[2], b.w[3]);
    have = 1;
    return u53(b.w[0], b.w[1]);
  }
  __device__ __forceinline__ double expo() { return -log(u()); }
  // Box-Muller on the next two uniforms (a, b): sqrt(-2 log a) cos(2 pi b); the sine value is not used
  __device__ __forceinline__ double normal() {
    const double a = u(), b = u();
    return sqrt(-2.0 * log(a)) * cos(6.283185307179586 * b);
  }
  __device__ __forceinline__ void bound_hit() { atomicOr(flags, FLAG_RNG_BOUND); }
};

// ---- the Monte-Carlo table of MCIntegrationVI (include/agp_hip.h, "MC INTEGRATION") ---------------------------------------------------
// Streams 2 (the gradient draw of step t) and 3 (the ELBO after t steps).  eps[s][k] is the contract's Normal of block 0 at counter
// (s K + k, t, stream, 0), with log and cos evaluated by the arithmetic below instead of the device's math library: every operation
// is one IEEE double operation (no contraction), so a host program that follows it gets the table bit for bit (tests/_mcvi_ref.py).
enum { RNG_STREAM_MC_GRAD = 2, RNG_STREAM_MC_ELBO = 3 };
// log(a), 0 < a < 1: a = m 2^e with sqrt(1/2) <= m < sqrt(2), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| < 0.1716: the odd series
// through s^23 / 23 by Horner in z = s^2, then e ln 2 + log m
__device__ __forceinline__ double mc_log(double a) {
#pragma clang fp contract(off)
  int e;
  double m = frexp(a, &e);
  if (m < 0.7071067811865476) {
    m = m * 2.0;
    e -= 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z + 1.0;
  return (double)e * 0.6931471805599453 + (2.0 * s) * p;
}
// cos(2 pi b), 0 < b < 1: folded exactly onto q in [0, 1/8] (1 - b, 1/2 - r, 1/4 - r are exact), then the Taylor polynomial of cos or
// sin at x = 2 pi q <= pi / 4 through x^16 / x^17 by Horner in x^2
__device__ __forceinline__ double mc_cos2pi(double b) {
#pragma clang fp contract(off)
  double r = b > 0.5 ? 1.0 - b : b;
  double sign = 1.0;
  if (r > 0.25) {
    r = 0.5 - r;
    sign = -1.0;
  }
  double v;
  if (r > 0.125) {
    const double x = 6.283185307179586 * (0.25 - r), z = x * x;
    double p = 1.0 / 355687428096000.0;              // 1 / 17!
    p = p * z - 1.0 / 1307674368000.0;               // 15!
    p = p * z + 1.0 / 6227020800.0;                  // 13!
    p = p * z - 1.0 / 39916800.0;                    // 11!
    p = p * z + 1.0 / 362880.0;                      // 9!
    p = p * z - 1.0 / 5040.0;
    p = p * z + 1.0 / 120.0;
    p = p * z - 1.0 / 6.0;
    p = p * z + 1.0;
    v = x * p;
  } else {
    const double x = 6.283185307179586 * r, z = x * x;
    double p = 1.0 / 20922789888000.0;               // 1 / 16!
    p = p * z - 1.0 / 87178291200.0;                 // 14!
    p = p * z + 1.0 / 479001600.0;                   // 12!
    p = p * z - 1.0 / 3628800.0;                     // 10!
    p = p * z + 1.0 / 40320.0;
    p = p * z - 1.0 / 720.0;
    p = p * z + 1.0 / 24.0;
    p = p * z - 1.0 / 2.0;
    p = p * z + 1.0;
    v = p;
  }
  return sign * v;
}
// out[i] = the Normal of counter (i, t, stream, 0), i < n = nMC K: the table double[nMC][K], filled once per step or evaluation
__global__ __launch_bounds__(256) void k_mc_normals(int64_t n, uint64_t seed, uint32_t t, uint32_t stream, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Philox4 b = philox4x32_10((uint32_t)i, t, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u0 = u53(b.w[0], b.w[1]), u1 = u53(b.w[2], b.w[3]);
  out[i] = sqrt(-2.0 * mc_log(u0)) * mc_cos2pi(u1);
}

constexpr double PG_T = 0.64;  // polyagamma.jl: pg_t

// log Phi(x) of the standard normal, without underflow in the lower tail
__device__ __forceinline__ double log_ndtr(double x) {
  const double s = x * 0.7071067811865476;
  return x < 0.0 ? log(0.5 * erfcx(-s)) - s * s : log1p(-0.5 * erfc(s));
}
// mass_texpon (polyagamma.jl:93-107): the probability of the truncated-exponential proposal
__device__ __noinline__ double pg_mass_texpon(double z) {
  const double K = 1.2337005501361697 + 0.5 * z * z;  // pi^2 / 8 + z^2 / 2
  const double b = 1.25 * (PG_T * z - 1.0), a = -1.25 * (PG_T * z + 1.0);  // sqrt(1 / t) = 1.25
  const double x0 = log(K) + K * PG_T;
  const double qdivp = 1.2732395447351628 * (exp(x0 - z + log_ndtr(b)) + exp(x0 + z + log_ndtr(a)));  // 4 / pi
  return 1.0 / (1.0 + qdivp);
}
// a(n, x) (polyagamma.jl:79-91)
__device__ __forceinline__ double pg_a(int n, double x) {
  const double h = (double)n + 0.5, k = h * 3.141592653589793;
  if (x > PG_T) return k * exp(-0.5 * k * k * x);
  return exp(-1.5 * (0.4515827052894548 + log(x)) + log(k) - 2.0 * h * h / x);  // log(pi / 2)
}
// truncated inverse Gaussian IG(1 / z, 1) on (0, t] (polyagamma.jl:110-137, with the second branch repeated until x <= t)
__device__ __forceinline__ double pg_tig(RngStream& s, double z) {
  const double mu = 1.0 / z;  // z = 0: inf, the first branch
  double x = 1.0 + PG_T;
  if (mu > PG_T) {
    for (int it = 0;; ++it) {
      double E = s.expo(), E2 = s.expo();
      for (int q = 0; E * E > 2.0 * E2 / PG_T; ++q) {
        if (q >= RNG_LOOP_MAX) {
          s.bound_hit();
          break;
        }
        E = s.expo();
        E2 = s.expo();
      }
      const double d = 1.0 + E * PG_T;
      x = PG_T / (d * d);
      const double alpha = exp(-0.5 * z * z * x);
      if (!(s.u() > alpha)) break;
      if (it >= RNG_LOOP_MAX) {
        s.bound_hit();
        break;
      }
    }
  } else {
    for (int it = 0;; ++it) {
      const double n = s.normal(), Y = n * n, muY = mu * Y;
      x = mu + 0.5 * mu * muY - 0.5 * mu * sqrt(4.0 * muY + muY * muY);
      if (s.u() > mu / (mu + x)) x = mu * mu / x;
      if (!(x > PG_T)) break;
      if (it >= RNG_LOOP_MAX) {
        s.bound_hit();
        x = PG_T;
        break;
      }
    }
  }
  return x;
}
// PG(1, c) by Devroye's alternating-series method (sample_pg1, polyagamma.jl:139-166); z = |c| / 2, r = pg_mass_texpon(z)
__device__ __forceinline__ double pg_draw1(RngStream& s, double z, double r) {
  const double K = 1.2337005501361697 + 0.5 * z * z;
  double x = PG_T;
  for (int it = 0;; ++it) {
    if (r > s.u())
      x = PG_T + s.expo() / K;
    else
      x = pg_tig(s, z);
    double S = pg_a(0, x);
    const double y = s.u() * S;
    bool accept = false;
    for (int n = 1;; ++n) {
      if (n > RNG_SERIES_MAX) {
        s.bound_hit();
        accept = true;
        break;
      }
      if (n & 1) {
        S -= pg_a(n, x);
        if (!(y > S)) {
          accept = true;
          break;
        }
      } else {
        S += pg_a(n, x);
        if (y > S) break;
      }
    }
    if (accept) break;
    if (it >= RNG_LOOP_MAX) {
      s.bound_hit();
      break;
    }
  }
  return 0.25 * x;
}
// PG(b, c), integer b >= 1: the sum of b draws of PG(1, c), each continuing the stream (draw_sum, polyagamma.jl:59-61)
__device__ __forceinline__ double pg_draw(RngStream& s, int64_t b, double c) {
  const double z = 0.5 * fabs(c), r = pg_mass_texpon(z);
  if (b > RNG_PG_B_MAX) {
    s.bound_hit();
    b = RNG_PG_B_MAX;
  }
  double sum = 0.0;
  for (int64_t k = 0; k < b; ++k) sum += pg_draw1(s, z, r);
  return sum;
}
// Gamma(alpha, 1) by Marsaglia & Tsang (2000), with the boost Gamma(alpha) = Gamma(alpha + 1) U^(1 / alpha) for alpha < 1
__device__ __forceinline__ double gamma_draw(RngStream& s, double alpha) {
  const double a1 = alpha < 1.0 ? alpha + 1.0 : alpha;
  const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double g = d;
  for (int it = 0;; ++it) {
    const double z = s.normal(), v1 = 1.0 + c * z;
    if (v1 > 0.0) {
      const double v = v1 * v1 * v1, u = s.u(), z2 = z * z;
      g = d * v;
      if (u < 1.0 - 0.0331 * z2 * z2) break;
      if (log(u) < 0.5 * z2 + d * (1.0 - v + log(v))) break;
    }
    if (it >= RNG_LOOP_MAX) {
      s.bound_hit();
      break;
    }
  }
  if (alpha < 1.0) g *= exp(log(s.u()) / alpha);
  return g;
}

// sample_local! of the three likelihoods (logistic.jl:53-60, studentt.jl:84-92, negativebinomial.jl:83-90) at f_i, then the
// expectation gradients of the SAME likelihood's AnalyticVI code (grad_E_mu, grad_E_Sigma = theta / 2) into r / w, where k_vgp_local
// writes them: k_vgp_eta then builds eta1 and -2 eta2 = inv(K) + 2 Diagonal(grad_E_Sigma) unchanged.  One lane per point; the
// rejection loops are lane-dependent.  aux: |f| (Logistic, NegBinomial) / the InverseGamma draw omega (StudentT: theta = 1 / omega).
// r, w and aux may be NULL (agp_sample_local: the sampler outside any model).
template <typename T>
__global__ __launch_bounds__(256) void k_gibbs_local(int64_t n, LikParams<T> lp, const T* __restrict__ y, const T* __restrict__ f,
                                                     uint64_t seed, uint32_t t, T* __restrict__ theta, T* __restrict__ aux,
                                                     T* __restrict__ r, T* __restrict__ w, int* __restrict__ flags) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  RngStream s(seed, t, RNG_STREAM_LOCAL, (uint32_t)i, flags);
  const double fi = (double)f[i], yi = (double)y[i];
  double th, ax, g1;
  if (lp.kind == LIK_STUDENTT) {
    const double nu = (double)lp.p0, sg = (double)lp.p1, alpha = 0.5 * (nu + 1.0);
    const double beta = 0.5 * ((fi - yi) * (fi - yi) + sg * sg * nu);
    ax = beta / gamma_draw(s, alpha);
    th = 1.0 / ax;
    g1 = th * yi;
  } else {
    int64_t b = 1;
    if (lp.kind != LIK_LOGISTIC) {
      if (!(yi >= 0.0 && yi == floor(yi))) atomicOr(flags, FLAG_BAD_COUNT);
      b = (int64_t)yi + (int64_t)lp.p0;
    }
    ax = fabs(fi);
    th = pg_draw(s, b, ax);
    g1 = lp.kind == LIK_LOGISTIC ? 0.5 * yi : 0.5 * (yi - (double)lp.p0);
  }
  theta[i] = (T)th;
  if (aux) aux[i] = (T)ax;
  if (r) {
    r[i] = (T)g1;
    w[i] = (T)(0.5 * th);
  }
}

// f = Xa' (v + z), z ~ N(0, I) from the normal stream (one block per point and sweep): with Xa = chol(-2 eta2)^-1 and v = Xa eta1 this
// is N(Sigma eta1, Sigma) (sample_global!, gibbssampling.jl:50-60).  The lower triangle of Xa is streamed once, like k_vgp_colstats:
// workgroup = 64 columns x 4 row phases of one row slice (blockIdx.y); part[s][col] = the slice's share of column col.  Rows >= m
// (the identity padding) carry z = 0.
template <typename T>
__global__ __launch_bounds__(256) void k_gibbs_f(int64_t m, int64_t mp, const T* __restrict__ X, const T* __restrict__ v,
                                                 int64_t rows_per_slice, uint64_t seed, uint32_t t, T* __restrict__ part,
                                                 int* __restrict__ flags) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 64, col = c0 + tx;
  const int64_t s = blockIdx.y;
  int64_t jlo = s * rows_per_slice;
  const int64_t jhi = jlo + rows_per_slice < mp ? jlo + rows_per_slice : mp;
  if (jlo < c0) jlo = c0;
  __shared__ T vz[256];
  __shared__ T sa[4][64];
  T a0 = T(0), a1 = T(0);
  for (int64_t j0 = jlo; j0 < jhi; j0 += 256) {  // (uniform over the workgroup)
    const int64_t jr = j0 + threadIdx.x;
    T val = T(0);
    if (jr < jhi) {
      val = v[jr];
      if (jr < m) {
        RngStream rs(seed, t, RNG_STREAM_NORMAL, (uint32_t)jr, flags);
        val += (T)rs.normal();
      }
    }
    vz[threadIdx.x] = val;
    __syncthreads();
    const int64_t je = jhi - j0 < 256 ? jhi - j0 : 256;
    int64_t q = ty;
    for (; q + 4 < je; q += 8) {  // two independent accumulators
      const int64_t j = j0 + q;
      const T x0 = j >= col ? X[j * mp + col] : T(0);
      const T x1 = j + 4 >= col ? X[(j + 4) * mp + col] : T(0);
      a0 += x0 * vz[q];
      a1 += x1 * vz[q + 4];
    }
    if (q < je) {
      const int64_t j = j0 + q;
      const T x0 = j >= col ? X[j * mp + col] : T(0);
      a0 += x0 * vz[q];
    }
    __syncthreads();
  }
  sa[ty][tx] = a0 + a1;
  __syncthreads();
  if (ty != 0) return;
  part[s * mp + col] = (sa[0][tx] + sa[1][tx]) + (sa[2][tx] + sa[3][tx]);
}
// ... the slices summed in order into f (the handle's state) and, for a kept sweep, into its row of the caller's sample store
template <typename T>
__global__ void k_gibbs_fsum(int64_t m, int64_t mp, int ns, const T* __restrict__ part, T* __restrict__ f, T* __restrict__ keep) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  T a = T(0);
  for (int s = 0; s < ns; ++s) a += part[s * mp + i];
  f[i] = a;
  if (keep) keep[i] = a;
}

// _predict_f(::MCGP) / proba_y(::MCGP) (predictions.jl:94-130, 260-276) per test point i from F*[i][s] = (K*n K^-1 f_s)_i, s < S:
//   mode 0  out0 = mean_s F*
//   mode 1  out0 = mean_s F*, out1 = k** + jitt - sum of the nsv row-dot slices pv (diag(K*n K^-1 Kn*)) + var_s F*
//   mode 2  out0, out1 = mean and variance over s of logistic(F*[i][s])
// var: the sample variance (n - 1), two passes.
template <typename T>
__global__ void k_mcgp_pred_finish(int64_t n, int S, const T* __restrict__ Fs, int64_t ldf, int mode, int nsv,
                                   const T* __restrict__ pv, int64_t ldp, T kdiag, T jitter, T* __restrict__ out0,
                                   T* __restrict__ out1) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const T* __restrict__ row = Fs + i * ldf;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) {
    const double x = (double)row[s];
    sum += mode == 2 ? (x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x))) : x;
  }
  const double mean = sum / (double)S;
  out0[i] = (T)mean;
  if (mode == 0) return;
  double ss = 0.0;
  for (int s = 0; s < S; ++s) {
    const double x = (double)row[s];
    const double d = (mode == 2 ? (x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x))) : x) - mean;
    ss += d * d;
  }
  const double var = S > 1 ? ss / (double)(S - 1) : __builtin_nan("");  // (one sample: NaN, like StatsBase.var)
  if (mode == 2) {
    out1[i] = (T)var;
    return;
  }
  double q = 0.0;
  for (int k = 0; k < nsv; ++k) q += (double)pv[k * ldp + i];
  out1[i] = (T)((double)kdiag + (double)jitter - q + var);
}

}  // namespace agp
