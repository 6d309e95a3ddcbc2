// Acquisition functions of the predictive moments and their multi-start ascent (agp_acq_moments, agp_svgp_acquisition,
// agp_svgp_acq_maximize; include/agp_hip.h "ACQUISITION FUNCTIONS").  Float64 only.
//   alpha(x) = A(mu(x), var(x)),  grad alpha = dA/dmu grad mu + dA/dvar grad var,   dA/dvar = dA/dsigma / (2 sigma)
// with mu, var the moments of agp_svgp_predict_f and grad mu, grad var those of agp_svgp_predict_f_grad (agp_predgrad.h): with
// t_ijd = s_d (x_id - z_jd), q_ij = sum_d t_ijd^2, k_ij = v phi(q_ij), c_ij = v phi'(q_ij), a and W = K*m Apred' of the predictor,
//   mu_i = sum_j a_j k_ij          dmu_i / dx_d  =  2 s_d sum_j a_j  c_ij t_ijd
//   u_i  = sum_j W_ij k_ij         dvar_i / dx_d = -4 s_d sum_j W_ij c_ij t_ijd          var_i = (v + jitter) - u_i
// k_acq_contract forms the four sums of a chunk of particles in one pass over the inducing-point tiles; k_acq_step / k_acq_finish add
// the column groups in ascending order and apply the point function.  No atomics: the order of every sum is fixed by (m, D).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_acq_log.h"  // acq_log_point: LogEI, LogPI
#include "agp_cavi.h"
#include "agp_hyper.h"
#include "agp_pathwise.h"  // PwAscentBox
#include "agp_predgrad.h"  // the tile geometry (PG_*, pg_ct, pg_tiles_per_group)

namespace agp {

// agp_acq_desc by value, with the sign of the objective resolved
struct AcqParams {
  int kind;            // AGP_ACQ_UCB = 0, AGP_ACQ_EI = 1, AGP_ACQ_PI = 2; AGP_ACQ_LOG_EI = 5, AGP_ACQ_LOG_PI = 6 (agp_acq_log.h)
  double s;            // +1, or -1 with minimize
  double beta, best, xi;
};

// The point function: alpha and its derivatives in mu and in var = sigma^2 (the table of include/agp_hip.h).  Phi(z) = erfc(-z /
// sqrt 2) / 2, never 1 + erf: EI lives in the left tail.  var <= 0 takes the defined limit (no 0 / 0), a NaN moment gives NaN.
// The kinds with the AGP_ACQ_LOG flag go to acq_log_point (agp_acq_log.h); what follows that line is UCB, EI and PI alone.
__device__ __forceinline__ void acq_point(const AcqParams& p, double mu, double var, double& alpha, double& dmu, double& dvar) {
#pragma clang fp contract(off)
  if (p.kind & 4) return acq_log_point(p.kind, p.s, p.best, p.xi, mu, var, alpha, dmu, dvar);
  if (mu != mu || var != var) {
    alpha = dmu = dvar = __builtin_nan("");
    return;
  }
  const double imp = p.s * (mu - p.best) - p.xi;  // the improvement before it is scaled (EI, PI)
  if (!(var > 0.0)) {
    dvar = 0.0;
    if (p.kind == 0) alpha = p.s * mu, dmu = p.s;
    else if (p.kind == 1) alpha = imp > 0.0 ? imp : 0.0, dmu = imp > 0.0 ? p.s : 0.0;
    else alpha = imp > 0.0 ? 1.0 : 0.0, dmu = 0.0;
    return;
  }
  const double sg = sqrt(var);
  if (p.kind == 0) {
    alpha = p.s * mu + p.beta * sg;
    dmu = p.s;
    dvar = p.beta / (2.0 * sg);
    return;
  }
  const double z = imp / sg;
  const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
  const double phi = 0.39894228040143267794 * exp(-0.5 * (z * z));
  if (p.kind == 1) {
    alpha = sg * (z * Phi + phi);
    dmu = p.s * Phi;
    dvar = phi / (2.0 * sg);
  } else {
    alpha = Phi;
    dmu = p.s * phi / sg;
    dvar = (-z * phi / sg) / (2.0 * sg);
  }
}

// agp_acq_moments: the point function alone on n given moments (dmu_out, dvar_out nullable)
__global__ void k_acq_moments(AcqParams p, int64_t n, const double* __restrict__ mu, const double* __restrict__ var,
                              double* __restrict__ alpha, double* __restrict__ dmu_out, double* __restrict__ dvar_out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a, dm, dv;
  acq_point(p, mu[i], var[i], a, dm, dv);
  alpha[i] = a;
  if (dmu_out) dmu_out[i] = dm;
  if (dvar_out) dvar_out[i] = dv;
}

// k_predgrad's structure (agp_predgrad.h): 64 particles per workgroup, lane = particle, one GROUP of inducing-point tiles per
// blockIdx.y, the four waves split a tile's columns in phase A and the input dimensions in phase B.
//   phase A  wave w, its CT/4 columns: q_ij by direct differences in ascending d, BOTH k_ij and c_ij from that q
//            (kernel_base_dbase), P0[j][i] = a_j c_ij, P1[j][i] = W_ij c_ij for phase B, and the wave's own sums of a_j k_ij and
//            W_ij k_ij over its columns in ascending j, one accumulator each, tiles ascending
//   phase B  wave w, its DPT dimensions: acc_d += P[j][i] t_ijd over the tile's columns in ascending j (mean and variance)
// After the last tile the four waves' scalar sums are added in ascending wave order through LDS.  The group's sums go, unscaled, to
//   part[0 | 1][group][i][d]   (group stride PG_CH rows; mean | variance: the layout of k_predgrad)
//   sc[0 | 1][group][i]        (mu-part | u-part)
// GRAD = false skips phase B and part (values only).  CT: 32 columns per tile, 16 at DPT = 16, as in k_predgrad, so the static LDS
// is that of k_predgrad<double, DPT, true> (56 KB at D = 64).  X rows >= nc are staged as zeros and never written; W is read for
// rows < nc and columns < m only.  variance < 0: the device-resident parameters (see k_kernelmatrix).
template <int DPT, bool GRAD>
__global__ void __launch_bounds__(PG_THREADS)
k_acq_contract(const double* __restrict__ X, int64_t ldx, int64_t nc, const double* __restrict__ Z, int64_t ldz, int64_t m, int D,
               const double* __restrict__ scales, int kind, double variance, const double* __restrict__ a,
               const double* __restrict__ W, int64_t ldw, int64_t tpg, double* __restrict__ part, double* __restrict__ sc) {
  constexpr int DP = 4 * DPT;
  constexpr int CT = pg_ct(DPT);
  constexpr int CW = CT / 4;
  __shared__ double xs[DP * PG_RT];
  __shared__ double zs[CT * DP];
  __shared__ double P[2 * CT * PG_RT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = blockIdx.x * (int64_t)PG_RT, gi = i0 + lane;
  const double var = variance < 0.0 ? scales[D] : variance;

  for (int e = tid; e < PG_RT * DP; e += PG_THREADS) {
    const int r = e / DP, d = e % DP;
    xs[d * PG_RT + r] = (d < D && i0 + r < nc) ? X[(i0 + r) * ldx + d] * scales[d] : 0.0;
  }
  __syncthreads();
  double xr[DPT], am[DPT], av[DPT];
#pragma unroll
  for (int k = 0; k < DPT; ++k) {
    xr[k] = xs[(w * DPT + k) * PG_RT + lane];
    am[k] = 0.0;
    av[k] = 0.0;
  }
  double smu = 0.0, su = 0.0;

  const int64_t jbeg = blockIdx.y * tpg * CT, jend = jbeg + tpg * CT < m ? jbeg + tpg * CT : m;
  for (int64_t j0 = jbeg; j0 < jend; j0 += CT) {
    __syncthreads();  // (phase B of the tile before has read zs and P)
    for (int e = tid; e < CT * DP; e += PG_THREADS) {
      const int j = e / DP, d = e % DP;
      zs[e] = (d < D && j0 + j < m) ? Z[(j0 + j) * ldz + d] * scales[d] : 0.0;
    }
    __syncthreads();
    {  // phase A
      double q[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) q[c] = 0.0;
      for (int d0 = 0; d0 < D; d0 += 4) {  // (the staged zeros beyond D add exact zeros)
#pragma unroll
        for (int d = d0; d < d0 + 4; ++d) {
          const double xv = xs[d * PG_RT + lane];
#pragma unroll
          for (int c = 0; c < CW; ++c) {
            const double t = xv - zs[(w * CW + c) * DP + d];
            q[c] = __builtin_fma(t, t, q[c]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const int jj = w * CW + c;
        const int64_t j = j0 + jj;
        double pm = 0.0, pv = 0.0;
        if (j < m) {
          double kb, kd;
          kernel_base_dbase<double>(kind, q[c], kb, kd);
          const double aj = a[j], wij = gi < nc ? W[gi * ldw + j] : 0.0;
          const double kij = var * kb, cij = var * kd;
          smu = __builtin_fma(aj, kij, smu);
          su = __builtin_fma(wij, kij, su);
          pm = aj * cij;
          pv = wij * cij;
        }
        if (GRAD) {
          P[jj * PG_RT + lane] = pm;
          P[(CT + jj) * PG_RT + lane] = pv;
        }
      }
    }
    if (GRAD) {
      __syncthreads();
      // phase B
#pragma unroll 4
      for (int jj = 0; jj < CT; ++jj) {
        const double pm = P[jj * PG_RT + lane];
        const double pv = P[(CT + jj) * PG_RT + lane];
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
          const double t = xr[k] - zs[jj * DP + w * DPT + k];
          am[k] = __builtin_fma(pm, t, am[k]);
          av[k] = __builtin_fma(pv, t, av[k]);
        }
      }
    }
  }
  __syncthreads();  // (the last tile's phase B has read P)
  P[w * PG_RT + lane] = smu;
  P[(4 + w) * PG_RT + lane] = su;
  __syncthreads();
  if (gi < nc) {
    if (w == 0) {
      double tm = 0.0, tu = 0.0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        tm += P[v * PG_RT + lane];
        tu += P[(4 + v) * PG_RT + lane];
      }
      sc[(int64_t)blockIdx.y * PG_CH + gi] = tm;
      sc[((int64_t)PG_MAXGROUPS + blockIdx.y) * PG_CH + gi] = tu;
    }
    if (GRAD) {
      double* pm = part + ((int64_t)blockIdx.y * PG_CH + gi) * D;
      double* pv = pm + (int64_t)PG_MAXGROUPS * PG_CH * D;
#pragma unroll
      for (int k = 0; k < DPT; ++k) {
        const int d = w * DPT + k;
        if (d < D) {
          pm[d] = am[k];
          pv[d] = av[k];
        }
      }
    }
  }
}

// the moments and the gradient component d of particle i from the groups' sums, groups in ascending order
__device__ __forceinline__ void acq_gather(int64_t i, int d, int D, int ng, const double* __restrict__ part,
                                           const double* __restrict__ sc, double kdiag_jit, double& mu, double& var, double& gm,
                                           double& gv) {
#pragma clang fp contract(off)
  double tm = 0.0, tu = 0.0;
  gm = 0.0, gv = 0.0;
  for (int g = 0; g < ng; ++g) {
    tm += sc[(int64_t)g * PG_CH + i];
    tu += sc[((int64_t)PG_MAXGROUPS + g) * PG_CH + i];
    if (part) {  // (NULL: values only)
      gm += part[((int64_t)g * PG_CH + i) * D + d];
      gv += part[(((int64_t)PG_MAXGROUPS + g) * PG_CH + i) * D + d];
    }
  }
  mu = tm;
  var = kdiag_jit - tu;
}

// agp_svgp_acquisition: alpha[i] and (grad nullable) grad[i][d] = dA/dmu 2 s_d gm + dA/dvar (-4 s_d) gv, one thread per (i, d); with
// grad = NULL (part = NULL too) one thread per point.  kdiag_jit = v + jitter, formed on the host as the predictor forms it.
__global__ void k_acq_finish(AcqParams p, int64_t nc, int D, int ng, const double* __restrict__ part, const double* __restrict__ sc,
                             const double* __restrict__ scales, double kdiag_jit, double* __restrict__ alpha, double* __restrict__ grad,
                             int64_t ldg) {
#pragma clang fp contract(off)
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int De = grad ? D : 1;
  if (e >= nc * De) return;
  const int64_t i = e / De;
  const int d = (int)(e % De);
  double mu, var, gm, gv, al, dm, dv;
  acq_gather(i, d, D, ng, grad ? part : nullptr, sc, kdiag_jit, mu, var, gm, gv);
  acq_point(p, mu, var, al, dm, dv);
  if (d == 0) alpha[i] = al;
  if (grad) {
    const double s = scales[d];
    grad[i * ldg + d] = dm * (2.0 * s * gm) + dv * (-4.0 * s * gv);
  }
}

// x = clip(x0), m = v = 0 of a chunk of particles (rows of x0 pitched by ldx0; the state is dense [np][D])
__global__ void k_acq_init(int64_t np, int D, const double* __restrict__ x0, int64_t ldx0, const PwAscentBox box, double* __restrict__ x,
                           double* __restrict__ mo, double* __restrict__ vo) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= np * D) return;
  const int64_t i = e / D;
  const int d = (int)(e % D);
  x[e] = fmin(fmax(x0[i * ldx0 + d], box.lo[d]), box.hi[d]);
  mo[e] = 0.0;
  vo[e] = 0.0;
}

// One ADAM step of agp_pathwise_maximize's recurrence on alpha (g = grad alpha: alpha is always maximised), one thread per (i, d);
// c1 = 1 - beta1^k, c2 = 1 - beta2^k come from the host's running products.  final != 0: the pass after the last step writes
// alpha[i] of the final iterate and leaves x, m, v alone.
__global__ void k_acq_step(AcqParams p, int64_t nc, int D, int ng, const double* __restrict__ part, const double* __restrict__ sc,
                           const double* __restrict__ scales, double kdiag_jit, double beta1, double beta2, double c1, double c2,
                           double eps, const PwAscentBox box, int final, double* __restrict__ x, double* __restrict__ mo,
                           double* __restrict__ vo, double* __restrict__ alpha) {
#pragma clang fp contract(off)
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int De = final ? 1 : D;
  if (e >= nc * De) return;
  const int64_t i = e / De;
  const int d = (int)(e % De);
  double mu, var, gm, gv, al, dm, dv;
  acq_gather(i, d, D, ng, final ? nullptr : part, sc, kdiag_jit, mu, var, gm, gv);
  acq_point(p, mu, var, al, dm, dv);
  if (final) {
    alpha[i] = al;
    return;
  }
  const double s = scales[d];
  const double gr = dm * (2.0 * s * gm) + dv * (-4.0 * s * gv);
  const int64_t o = i * D + d;
  const double m1 = beta1 * mo[o] + (1.0 - beta1) * gr;
  const double v1 = beta2 * vo[o] + (1.0 - beta2) * (gr * gr);
  mo[o] = m1;
  vo[o] = v1;
  const double xn = x[o] + box.lr[d] * ((m1 / c1) / (sqrt(v1 / c2) + eps));
  x[o] = fmin(fmax(xn, box.lo[d]), box.hi[d]);
}

}  // namespace agp
