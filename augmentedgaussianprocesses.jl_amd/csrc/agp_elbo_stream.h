// Streamed full-data ELBO (agp_svgp_elbo_stream, include/agp_hip.h "STREAMED ELBO"): the point-wise kernel that turns a chunk's
// (mean_f, var_f) into per-workgroup partial sums of the two data terms, and the fixed-order reduction over all partials.
#pragma once
#include "agp_cavi.h"

namespace agp {

constexpr int ELBO_STREAM_THREADS = 256;
constexpr unsigned long long ELBO_STREAM_NONE = ~0ull;  // "no such point" in the two failure words

// One lane per point of a chunk of nc points that starts at global point `base`; mu / var are the chunk's moments [nl][ldc] from
// the predictor's chunk loop.  The fresh local variables of the point (ELBO.jl:32-47: new local variables, ONE local update) are
// formed in registers -- lik_point for the single-latent likelihoods; for LogisticSoftMax alpha = n_class, c_k, two rounds of
// (gamma, alpha) and the final theta, operation for operation what k_rowstats_local + k_lsm_gamma / k_lsm_alpha / k_lsm_finish leave
// in the step's buffers (gamma_k is re-evaluated per pass instead of kept: exp(psi(alpha)) changes between the rounds, the
// exp / cosh factor does not, and no per-latent array has to live across the passes, so any number of latents stays in registers).
// The two per-point terms are elbo_point_terms / elbo_lsm_latent, in double, as in k_elbo_terms.
// part[2 w], part[2 w + 1] = block_sum of the workgroup's points, w = its index within the chunk (the caller offsets `part` by the
// chunk's first workgroup): no atomics on floating-point values, nothing depends on which CU ran which workgroup.
// bad[0] = smallest global index of a point whose var_f is not > 0 or whose moments are not finite; bad[1] = smallest global index
// of a LogisticSoftMax label outside [0, n_class).  Such a point adds nothing to the sums (the call fails).
template <typename T, int KIND>
__global__ void __launch_bounds__(ELBO_STREAM_THREADS)
k_elbo_stream_terms(int64_t nc, int64_t base, int nl, int64_t ldc, LikParams<T> lp, int elbo_ref, const T* __restrict__ y,
                    const int32_t* __restrict__ ycls, const int64_t* __restrict__ idx, const T* __restrict__ mu,
                    const T* __restrict__ var, int n_class, double* __restrict__ part, unsigned long long* __restrict__ bad) {
  __shared__ double red[ELBO_STREAM_THREADS / 64];
  const int64_t i = blockIdx.x * (int64_t)ELBO_STREAM_THREADS + threadIdx.x;
  double e = 0.0, kl = 0.0;
  if (i < nc) {
    const int64_t gi = base + i;                 // position in the stream
    const int64_t row = idx ? idx[gi] : gi;      // row of y (and of x, gathered by the kernel-matrix kernel)
    bool ok = true;
    for (int k = 0; k < nl; ++k) {
      const T mk = mu[k * ldc + i], vk = var[k * ldc + i];
      ok = ok && (vk > T(0)) && (fabs(mk) < (T)__builtin_inf()) && (vk < (T)__builtin_inf());
    }
    if (!ok) {
      atomicMin(&bad[0], (unsigned long long)gi);
    } else if constexpr (KIND == LIK_LSM) {
      const int cls = ycls[row];
      if (cls < 0 || cls >= n_class) atomicMin(&bad[1], (unsigned long long)gi);
      const T beta = (T)n_class;  // init_local_vars, logisticsoftmax.jl:43-53 (beta is never updated)
      const double b2 = 2.0 * (double)beta;
      T a = (T)n_class;
      for (int it = 0; it < 2; ++it) {  // logisticsoftmax.jl:65-72
        const double epsi = exp(digamma_d((double)a));
        double s = 0.0;
        for (int k = 0; k < nl; ++k) {
          const T mk = mu[k * ldc + i], vk = var[k * ldc + i];
          const T ck = sqrt(mk * mk + vk);
          s += epsi * safe_expcosh_d(-0.5 * (double)mk, 0.5 * (double)ck) / b2;
        }
        if (it == 1) {
          // the terms want gamma of THIS round (k_lsm_gamma's) next to alpha of after it (k_lsm_alpha's)
          const double an = (double)(T(1) + (T)s);
          const double psi = digamma_d(an);
          const double lam0 = an / (double)beta, psil = psi - log((double)beta);
          for (int k = 0; k < nl; ++k) {
            const T mk = mu[k * ldc + i], vk = var[k * ldc + i];
            const T ck = sqrt(mk * mk + vk);
            const T g = (T)(epsi * safe_expcosh_d(-0.5 * (double)mk, 0.5 * (double)ck) / b2);
            const T yk = (cls == k) ? T(1) : T(0);
            const T th = (yk + g) * theta_pg<T>(ck);  // k_lsm_finish
            elbo_lsm_latent((double)yk, (double)g, (double)th, (double)mk, (double)vk, (double)ck, lam0, psil, e, kl);
          }
          elbo_lsm_entropy(an, psi, kl);
        }
        a = T(1) + (T)s;
      }
    } else {
      const T mk = mu[i], vk = var[i], yi = y[row];
      T th, cc, g1;
      lik_point<T>(KIND, lp.p0, lp.p1, mk, vk, yi, th, cc, g1);
      const ElboConsts kc = elbo_consts<T, KIND>(lp, (double)lp.p0, 1.0);
      elbo_point_terms<T, KIND>(lp, elbo_ref, kc, gi == 0, (double)yi, (double)mk, (double)vk, (double)th, (double)cc, e, kl);
    }
  }
  e = block_sum<double>(e, red);
  kl = block_sum<double>(kl, red);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = e;
    part[2 * (int64_t)blockIdx.x + 1] = kl;
  }
}

// out[0], out[1] = the sums of part[2 w], part[2 w + 1] over all nw workgroups of all chunks, in ONE fixed order: thread t adds
// the partials t, t + 1024, ... in that order, then block_sum.  once_add (log(beta[0]) of LogisticSoftMax, counted once per
// evaluation) joins out[1].  out[2], out[3] = the two failure words as doubles (an index < 2^53), -1 = none.
__global__ void __launch_bounds__(1024)
k_elbo_stream_reduce(const double* __restrict__ part, int64_t nw, double once_add, const unsigned long long* __restrict__ bad,
                     double* __restrict__ out) {
  __shared__ double red[16];
  double e = 0.0, kl = 0.0;
  for (int64_t w = threadIdx.x; w < nw; w += blockDim.x) {
    e += part[2 * w];
    kl += part[2 * w + 1];
  }
  e = block_sum<double>(e, red);
  kl = block_sum<double>(kl, red);
  if (threadIdx.x == 0) {
    out[0] = e;
    out[1] = kl + once_add;
    out[2] = bad[0] == ELBO_STREAM_NONE ? -1.0 : (double)bad[0];
    out[3] = bad[1] == ELBO_STREAM_NONE ? -1.0 : (double)bad[1];
  }
}

}  // namespace agp
