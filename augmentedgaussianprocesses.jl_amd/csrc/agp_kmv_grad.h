// agp_kmv_grad.h -- the derivative bilinear form of the matrix-free kernel operator (agp_kmv.h): for G_ij = sum_c w_c U_ic V_jc (r <= 32
// weighted pairs of vectors), t_ijd = s_d (x_id - x_jd) and c_ij = G_ij variance phi'(d2_ij),
//     dvar     = sum_ij G_ij phi(d2_ij)                  ( = sum_c w_c u_c' (dK / d variance) v_c )
//     dscale_d = (2 / s_d) sum_ij c_ij t_ijd^2           ( = sum_c w_c u_c' (dK / d s_d) v_c )
// with neither K nor G (both n x n) in memory or LDS.  Symmetric use only (Y = X, the prepared KmvOp).  Float64, D <= 64.
// These are the two traces of the log marginal likelihood's gradient, 1/2 alpha'(dK)alpha and -1/2 tr((K + s2 I)^-1 dK) by probes.
//
// k_kmv_grad -- k_kmv's work split (one workgroup of 4 waves per 64-row tile and column group, wave w owns rows 16 w .. 16 w + 15),
// its register prefetch and its fixed summation orders, with three products per 32 columns of a tile instead of two:
//   d2 step     S' = Ys Xs' as in k_kmv (X fragments resident in registers), the KMM_CLOSE repair, d2 = 0 on the diagonal.
//   G step      G' = Vs (diag(w) Us)' on the same instruction: A operand = the V tile staged in LDS as [j][c] with row stride R + 2 (the
//               operand-tile stride rule of Ys), B operand = the wave's 16 rows of U times w, resident for the whole launch (R / 4
//               doubles per lane).  G lands in the accumulator layout of S': element q of g[h] and of s[h] are the same (i, j).
//   function    phi and phi' from one exponential (kmv_phi_dphi) on the accumulators; G phi goes to the lane's private dvar partial, the accumulator becomes
//               c = G variance phi' (0 on the diagonal, where t = 0), and the lane adds c to its row-sum partial rho.
//   product     c already has the A-operand layout (k_kmv's register hand-over): O += C sY and Q += C (sY o sY), B operand read from the
//               Y tile that is in LDS anyway, squared in registers.  Two independent accumulator chains per 16 dimensions.
// At the end of the walk  sum_j c_ij t_ijd^2 = sx_id^2 rho_i + Q_id - 2 sx_id O_id ; the 64 rows are added in a fixed order (q, then
// (wave, lane >> 4) ascending) and the workgroup writes ONE partial of 1 + D doubles.  k_kmv_grad_sum adds the partials in a fixed order.
// No atomics: two calls agree bit for bit.  The expanded form cancels where points are close: its absolute error scales with
// sum_ij |c_ij| (|sx_id| + |sx_jd|)^2, not with the result (DESIGN.md 9q has the budget).
// LDS (doubles): 2 x 64 (DP + 2) operand tiles + 64 (R + 2) for V + 128 norms + DP scales; the end-of-walk reduction reuses the Y tile.
#pragma once
#include "agp_hyper.h"  // kernel_base_dbase
#include "agp_kmv.h"

namespace agp {

struct KmvGradW {
  double w[KMV_MAXR];
};
template <int DP, int RB>
constexpr size_t kmv_grad_smem_bytes() {
  return sizeof(double) * (size_t)(2 * TILE * (DP + 2) + TILE * (16 * RB + 2) + 2 * TILE + DP);
}

// phi and phi' with ONE exponential for every kind (kernel_base_dbase has one for the squared exponential only; with its two the
// Matern-5/2 form at DP = 32, R = 32 carried 32 bytes of scratch per lane).  Same expressions as kernel_base / kernel_dbase.
template <int KIND>
__device__ __forceinline__ void kmv_phi_dphi(double d2, double& base, double& dbase) {
  if constexpr (KIND == K_SQEXP) {
    kernel_base_dbase<double>(K_SQEXP, d2, base, dbase);
  } else {
    d2 = d2 > 0.0 ? d2 : 0.0;
    const double r = sqrt(d2);
    if constexpr (KIND == K_MATERN52) {
      const double s5 = 2.23606797749978969641, e = exp_nonpos(-s5 * r);
      base = (1.0 + s5 * r + 5.0 * d2 / 3.0) * e;
      dbase = -(5.0 / 6.0) * (1.0 + s5 * r) * e;
    } else {
      const double s3 = 1.73205080756887729353, e = exp_nonpos(-s3 * r);
      base = (1.0 + s3 * r) * e;
      dbase = -1.5 * e;
    }
  }
}

// grid = (column groups, row tiles); part: [group][row tile][1 + D]
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, DP == 64 ? 1 : 2) void k_kmv_grad(const double* __restrict__ X, int64_t ldx, int64_t n,
                                                                         const double* __restrict__ Ysc,
                                                                         const double* __restrict__ yng, int64_t D,
                                                                         const double* __restrict__ scales, double variance,
                                                                         const double* __restrict__ U, int64_t ldu,
                                                                         const double* __restrict__ V, int64_t ldv, int r,
                                                                         KmvGradW wts, double* __restrict__ part) {
  constexpr int LDX = DP + 2, R = 16 * RB, LDG = R + 2, NK = DP / 4, NG = R / 4, NB = DP / 16, YQ = DP / 8, VQ = 4 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char kmv_smem[];
  double* Xs = reinterpret_cast<double*>(kmv_smem);  // [64][LDX]
  double* Ys = Xs + TILE * LDX;                      // [64][LDX]
  double* Vs = Ys + TILE * LDX;                      // [64][LDG]
  double* xn = Vs + TILE * LDG;                      // [64]
  double* yn = xn + TILE;                            // [64]
  double* sc = yn + TILE;                            // [DP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  const int64_t nct = (n + TILE - 1) / TILE, base = nct / gridDim.x, rem = nct % gridDim.x;
  const int64_t ct0 = blockIdx.x * base + ((int64_t)blockIdx.x < rem ? blockIdx.x : rem);
  const int64_t ct1 = ct0 + base + ((int64_t)blockIdx.x < rem ? 1 : 0);

  d2v yr[YQ];
  double vr[VQ], ynr = 0.0;
  auto fetch = [&](int64_t ct) {
    const double* src = Ysc + ct * TILE * DP;
#pragma unroll
    for (int q = 0; q < YQ; ++q) yr[q] = *reinterpret_cast<const d2v*>(src + (int64_t)(tid + NTHREADS * q) * 2);
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = ct * TILE + j;
      vr[q] = (gj < n && c < r) ? V[gj * ldv + c] : 0.0;
    }
    if (tid < TILE) ynr = yng[ct * TILE + tid];
  };
  if (ct0 < ct1) fetch(ct0);

  for (int d = tid; d < DP; d += NTHREADS) sc[d] = d < D ? scales[d] : 0.0;
  __syncthreads();
  for (int e = tid; e < TILE * DP; e += NTHREADS) {
    const int rr = e / DP, d = e % DP;
    const int64_t gr = i0 + rr;
    Xs[rr * LDX + d] = (gr < n && d < D) ? X[gr * ldx + d] * sc[d] : 0.0;
  }
  __syncthreads();
  {
    const int rr = tid >> 2, q4 = tid & 3;
    double s = 0.0;
    for (int d = q4; d < DP; d += 4) s += Xs[rr * LDX + d] * Xs[rr * LDX + d];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (q4 == 0) xn[rr] = s;
  }
  __syncthreads();
  const int il = wave * 16 + l15;  // this lane's row of the tile in the d2, G and function steps
  double xb[NK], ub[NG];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) xb[kk] = Xs[il * LDX + kk * 4 + l4];
#pragma unroll
  for (int kk = 0; kk < NG; ++kk) {  // the wave's rows of U diag(w): B operand of the G step
    const int c = kk * 4 + l4;
    ub[kk] = (i0 + il < n && c < r) ? U[(i0 + il) * ldu + c] * wts.w[c] : 0.0;
  }
  const double xnv = xn[il];
  const double close_thr = KMM_CLOSE<double>;

  d4 o[NB], qq[NB];
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[db][q] = qq[db][q] = 0.0;
  double dv = 0.0, rho = 0.0;

  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t j0 = ct * TILE;
    if (ct != ct0) __syncthreads();  // the previous tile's products are done with Ys / Vs / yn
#pragma unroll
    for (int q = 0; q < YQ; ++q) {
      const int e = tid + NTHREADS * q, row = e / (DP / 2), v = e % (DP / 2);
      *reinterpret_cast<d2v*>(Ys + row * LDX + 2 * v) = yr[q];
    }
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q;
      Vs[(e / R) * LDG + (e % R)] = vr[q];
    }
    if (tid < TILE) yn[tid] = ynr;
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products

    const double* pa = Ys + l15 * LDX + l4;
    const double* pg = Vs + l15 * LDG + l4;
    const double* py = Ys + l4 * LDX + l15;
    const int64_t dg = (i0 + il) - j0;  // the local column of the diagonal element of this row, if in this tile
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {  // (rolled for the reason given in k_kmv)
      d4 s[2], g[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[h][q] = g[h][q] = 0.0;
      const double* pj = pa + jp * 32 * LDX;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double a = pj[h * 16 * LDX + kk * 4];
          lds_keep_apart();
          s[h] = Mfma<double>::mma(a, xb[kk], s[h]);
        }
      const double* pw = pg + jp * 32 * LDG;
#pragma unroll
      for (int kk = 0; kk < NG; ++kk)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double a = pw[h * 16 * LDG + kk * 4];
          lds_keep_apart();
          g[h] = Mfma<double>::mma(a, ub[kk], g[h]);
        }
      // function step: element q of s[h] and g[h] is (row il, column 32 jp + 16 h + l4 + 4 q)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jp * 32 + h * 16 + l4 + 4 * q;
          const bool diag = (int64_t)jl == dg;
          const double s2 = xnv + yn[jl];
          double d2 = s2 - 2.0 * s[h][q];
          if (diag) {
            d2 = 0.0;
          } else if (d2 < close_thr * s2) {
            double t = 0.0;
#pragma unroll 1
            for (int d = 0; d < DP; ++d) {
              const double df = Xs[il * LDX + d] - Ys[jl * LDX + d];
              t += df * df;
            }
            d2 = t;
          }
          double kb, kd;
          kmv_phi_dphi<KIND>(d2, kb, kd);
          dv = __builtin_fma(g[h][q], kb, dv);
          const double c = diag ? 0.0 : g[h][q] * variance * kd;  // (t = 0 on the diagonal: it has no share in dscale)
          rho += c;
          s[h][q] = c;
        }
      // third product: k-step 8 jp + 4 h + q takes c = s[h][q] as its A operand as it stands
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int db = 0; db < NB; ++db) {
            const double b = py[(jp * 32 + h * 16 + q * 4) * LDX + db * 16];
            lds_keep_apart();
            o[db] = Mfma<double>::mma(s[h][q], b, o[db]);
            qq[db] = Mfma<double>::mma(s[h][q], b * b, qq[db]);
          }
    }
  }
  // ---- end of the walk: rho over the four lanes of a row, then sx^2 rho + Q - 2 sx O summed over the 64 rows ----
  rho += __shfl_xor(rho, 16);
  rho += __shfl_xor(rho, 32);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) dv += __shfl_xor(dv, off);
  __syncthreads();  // every wave is done with Ys / yn / xn
  if (l4 == 0) xn[il] = rho;
  if (lane == 0) yn[wave] = dv;
  __syncthreads();
  double* red = Ys;  // [16][DP]: the partial of (wave, l4) over its four rows
#pragma unroll
  for (int db = 0; db < NB; ++db) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // element q of o[db]: row wave * 16 + l4 + 4 q, dimension 16 db + l15
      const int row = wave * 16 + l4 + 4 * q;
      const double sx = Xs[row * LDX + db * 16 + l15];
      acc += __builtin_fma(sx * sx, xn[row], qq[db][q]) - 2.0 * sx * o[db][q];
    }
    red[(wave * 4 + l4) * DP + db * 16 + l15] = acc;
  }
  __syncthreads();
  double* dst = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (1 + D);
  if (tid < D) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k * DP + tid];
    dst[1 + tid] = (2.0 / sc[tid]) * t;
  }
  if (tid == NTHREADS - 1) dst[0] = ((yn[0] + yn[1]) + yn[2]) + yn[3];
}

// out[e] = sum_b part[b][e], e < 1 + D: one workgroup per e; thread t adds b = t, t + 256, ... in ascending order and thread 0 the 256
// sums in ascending t -- a fixed order for a given launch geometry
__global__ __launch_bounds__(256) void k_kmv_grad_sum(const double* __restrict__ part, int64_t nparts, int64_t width,
                                                      double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x, e = blockIdx.x;
  double s = 0.0;
  for (int64_t b = tid; b < nparts; b += 256) s += part[b * width + e];
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < 256; ++k) t += red[k];
    out[e] = t;
  }
}

}  // namespace agp
