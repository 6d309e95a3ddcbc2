// Input gradients of the predictive moments (agp_svgp_predict_f_grad, include/agp_hip.h "PREDICTIVE GRADIENTS"; DESIGN.md section
// 9n).  With t_ijd = s_d (x_id - z_jd), q_ij = sum_d t_ijd^2 and c_ij = variance * phi'(q_ij) (kernel_dbase, agp_hyper.h: the forms that
// are finite at r = 0 and never divide by r),
//   dmu_i  / dx_d =  2 s_d sum_j  a_j   c_ij t_ijd          a = K^-1 mu       (the predictor's apred)
//   dvar_i / dx_d = -4 s_d sum_j  W_ij  c_ij t_ijd          W = K*m A          (the predictor's Apred; k** + jitter is constant in x)
// One kernel forms both: a fused "evaluate c, scale, contract with the differences" over the inducing-point tiles.  A coinciding pair
// x_i = z_j has t = 0 exactly and adds exactly 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agp_cavi.h"
#include "agp_hyper.h"

namespace agp {

constexpr int PG_THREADS = 256;
constexpr int PG_RT = 64;          // test points per workgroup: one per lane
constexpr int PG_MAXD = HB_MAXD;   // the hyper-gradient's limit on the input dimension (agp_hip.h)

// A workgroup carries PG_RT = 64 test points through ONE GROUP of inducing-point tiles (blockIdx.y; `tpg` tiles of CT columns each);
// lane = point, the four waves split the columns of a tile in phase A and the input dimensions in phase B.  DPT = dimensions per
// wave (1, 4, 8, 16: D <= 4 DPT).
//   stage    zs[j][d] = s_d z_jd of the tile (xs[d][i] = s_d x_id once per workgroup), in double for both dtypes, zero beyond m / D
//   phase A  wave w, columns w CT/4 .. : q_ij = sum_d (xs - zs)^2 in ASCENDING d, as k_kernelmatrix sums it (direct differences: no
//            GEMM-form cancellation), then P0[j][i] = a_j c_ij (and P1[j][i] = W_ij c_ij)
//   phase B  wave w, dimensions w DPT .. : acc_d += P[j][i] (xs_id - zs[j][d]) over the tile's columns in ascending j
// and leaves the group's sums, unscaled and in double, in part[0 | 1][group][i][d] (mean | variance; group stride PG_CH rows).
// k_predgrad_finish adds the groups in ascending order and applies 2 s_d resp. -4 s_d.  The split into groups is a function of m
// and D alone (pg_tiles_per_group), so the order of every sum is fixed by (m, D): no atomics, the same bits on every call and for
// every position of a point in the stream.  The groups are there for occupancy: a chunk of 4096 points is only 64 row tiles.
// LDS reads: P lane-strided (conflict-free), zs one address per wave (broadcast), xs lane-strided.  At D = 32 phase B issues 24
// v_*_f64 per wave and column against 20 LDS cycles; CT drops to 16 at DPT = 16 so that every variant stays under 64 KB of static
// LDS (56 KB at D = 64: two workgroups per CU).
// X rows >= nc are staged as zeros and never written; W (ldw) is read for rows < nc and columns < m only; part is written for rows
// < nc and d < D only.  variance < 0: the device-resident parameters (see k_kernelmatrix).
constexpr int PG_CH = 4096;      // points per chunk of the stream (the predictor's)
constexpr int PG_MAXGROUPS = 8;  // column groups of a row tile
__host__ __device__ constexpr int pg_ct(int dpt) { return dpt == 16 ? 16 : 32; }  // inducing points per tile
// tiles per group: at least two, at most PG_MAXGROUPS groups (m = 1024 at D <= 32: 32 tiles, 8 groups of 4)
static inline int64_t pg_tiles_per_group(int64_t m, int dpt) {
  const int64_t nt = (m + pg_ct(dpt) - 1) / pg_ct(dpt), t = (nt + PG_MAXGROUPS - 1) / PG_MAXGROUPS;
  return t < 2 ? 2 : t;
}
template <typename T, int DPT, bool VAR>
__global__ void __launch_bounds__(PG_THREADS)
k_predgrad(const T* __restrict__ X, int64_t ldx, int64_t nc, const T* __restrict__ Z, int64_t ldz, int64_t m, int D,
           const T* __restrict__ scales, int kind, T variance, const T* __restrict__ a, const T* __restrict__ W, int64_t ldw,
           int64_t tpg, double* __restrict__ part) {
  constexpr int DP = 4 * DPT;      // staged dimensions (zero beyond D)
  constexpr int CT = pg_ct(DPT);
  constexpr int CW = CT / 4;               // columns per wave in phase A
  __shared__ double xs[DP * PG_RT];
  __shared__ double zs[CT * DP];
  __shared__ double P[(VAR ? 2 : 1) * CT * PG_RT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = blockIdx.x * (int64_t)PG_RT, gi = i0 + lane;
  const double var = variance < T(0) ? (double)scales[D] : (double)variance;

  for (int e = tid; e < PG_RT * DP; e += PG_THREADS) {
    const int r = e / DP, d = e % DP;
    xs[d * PG_RT + r] = (d < D && i0 + r < nc) ? (double)X[(i0 + r) * ldx + d] * (double)scales[d] : 0.0;
  }
  __syncthreads();
  double xr[DPT], am[DPT], av[DPT];
#pragma unroll
  for (int k = 0; k < DPT; ++k) {
    xr[k] = xs[(w * DPT + k) * PG_RT + lane];
    am[k] = 0.0;
    av[k] = 0.0;
  }

  const int64_t jbeg = blockIdx.y * tpg * CT, jend = jbeg + tpg * CT < m ? jbeg + tpg * CT : m;
  for (int64_t j0 = jbeg; j0 < jend; j0 += CT) {
    __syncthreads();  // (phase B of the tile before has read zs and P)
    for (int e = tid; e < CT * DP; e += PG_THREADS) {
      const int j = e / DP, d = e % DP;
      zs[e] = (d < D && j0 + j < m) ? (double)Z[(j0 + j) * ldz + d] * (double)scales[d] : 0.0;
    }
    __syncthreads();
    {  // phase A
      double q[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) q[c] = 0.0;
      // four dimensions per trip, so that their LDS reads are in flight together (the staged zeros beyond D add exact zeros)
      for (int d0 = 0; d0 < D; d0 += 4) {
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
          const double cij = var * kernel_dbase<double>(kind, q[c]);
          pm = (double)a[j] * cij;
          if (VAR && gi < nc) pv = (double)W[gi * ldw + j] * cij;
        }
        P[jj * PG_RT + lane] = pm;
        if (VAR) P[(CT + jj) * PG_RT + lane] = pv;
      }
    }
    __syncthreads();
    // phase B
#pragma unroll 4
    for (int jj = 0; jj < CT; ++jj) {
      const double pm = P[jj * PG_RT + lane];
      const double pv = VAR ? P[(CT + jj) * PG_RT + lane] : 0.0;
#pragma unroll
      for (int k = 0; k < DPT; ++k) {
        const double t = xr[k] - zs[jj * DP + w * DPT + k];
        am[k] = __builtin_fma(pm, t, am[k]);
        if (VAR) av[k] = __builtin_fma(pv, t, av[k]);
      }
    }
  }
  if (gi < nc) {
    double* pm = part + ((int64_t)blockIdx.y * PG_CH + gi) * D;
    double* pv = pm + (int64_t)PG_MAXGROUPS * PG_CH * D;
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
      const int d = w * DPT + k;
      if (d < D) {
        pm[d] = am[k];
        if (VAR) pv[d] = av[k];
      }
    }
  }
}

// dmu[i][d] = 2 s_d sum_g part[0][g][i][d], dvar[i][d] = -4 s_d sum_g part[1][g][i][d] (dvar nullable), groups in ascending order;
// rows pitched by ldo, d < D only.
template <typename T>
__global__ void k_predgrad_finish(int64_t nc, int D, int ng, const double* __restrict__ part, const T* __restrict__ scales,
                                  T* __restrict__ dmu, T* __restrict__ dvar, int64_t ldo) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= nc * D) return;
  const int64_t i = e / D;
  const int d = (int)(e % D);
  const double s = (double)scales[d];
  const double* pv = part + (int64_t)PG_MAXGROUPS * PG_CH * D;
  double sm = 0.0, sv = 0.0;
  for (int g = 0; g < ng; ++g) {
    sm += part[((int64_t)g * PG_CH + i) * D + d];
    if (dvar) sv += pv[((int64_t)g * PG_CH + i) * D + d];
  }
  dmu[i * ldo + d] = (T)(2.0 * s * sm);
  if (dvar) dvar[i * ldo + d] = (T)(-4.0 * s * sv);
}

// multi-output handles: out[t][i][d] = sum_q A[t][q]^p in[q][i][d] (p = 1 means, p = 2 variances; predictions.jl:60-64,75-79 applied
// to the gradients), in = T[Q][ldi][D] dense, out rows pitched by ldo, latent stride lso.  Accumulated in double, ascending q.
template <typename T>
__global__ void k_predgrad_mix(int64_t nc, int D, int Q, int nT, const T* __restrict__ A, int lda, const T* __restrict__ in,
                               int64_t ldi, T* __restrict__ out, int64_t ldo, int64_t lso, int square) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= nc * D) return;
  const int64_t i = e / D;
  const int d = (int)(e % D);
  for (int t = 0; t < nT; ++t) {
    double s = 0.0;
    for (int q = 0; q < Q; ++q) {
      const double aq = (double)A[t * lda + q];
      s += (square ? aq * aq : aq) * (double)in[((int64_t)q * ldi + i) * D + d];
    }
    out[t * lso + i * ldo + d] = (T)s;
  }
}

}  // namespace agp
