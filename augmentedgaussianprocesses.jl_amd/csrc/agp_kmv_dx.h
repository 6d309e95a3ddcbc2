// agp_kmv_dx.h -- the derivative of the matrix-free kernel operator (agp_kmv.h) with respect to its ROW points: for k = variance phi(d2),
// t_ijd = s_d (x_id - y_jd) and c_ij = variance phi'(d2_ij), d k(x_i, y_j) / d x_id = 2 s_d c_ij t_ijd, and
//     shared   Out[i][c][d] = 2 s_d sum_j c_ij V_jc t_ijd       V: p x r, r <= 32 (the mean gradient, r function draws)
//     paired   Out[i][d]    = 2 s_d sum_j c_ij V_ji t_ijd       V: p x n, n <= 32: row i uses column i of V (the variance gradient)
// with neither K nor dK / dx (n x p x D) in memory.  Cross form only (X and Y are different point sets; a row point that coincides with
// a column point is an ordinary input: t = 0, it contributes 0).  Float64, D <= 64, squared exponential and Matern-3/2, -5/2.
//
// k_kmv_dx<KIND, DP, CB, PAIRED> -- k_kmv's work split (one workgroup of 4 waves per 64-row tile of X and column group of Y, wave w owns
// rows 16 w .. 16 w + 15, next tile prefetched into registers) with a THIRD grid dimension over blocks of CB right-hand sides: the
// accumulators of ONE right-hand side are 16 x DP per wave (DP / 16 MFMA tiles, DP / 4 doubles per lane), so 32 of them cannot be
// resident at once, and every column block recomputes d2 and phi'.
//   d2 step     S' = Ys Xs' as in k_kmv: A operand = the Y tile in LDS (row stride DP + 2), B operand = the wave's X rows, resident in
//               registers; the KMM_CLOSE repair by direct differences from the tiles in LDS.
//   function    c = variance phi' on the accumulators (phi is not needed: one exponential per element).  For each right-hand side of
//               the block the lane multiplies c_ij by V_jc -- paired: by V_ji -- read from the V tile in LDS at the lane's own (i, j),
//               and adds the product to its private row sum rho_ic.
//   product     c o v_c already has the A-operand layout (k_kmv's register hand-over): O_c += (C o v_c) (sY - m), B operand read from
//               a SECOND copy of the Y tile with a row stride of its own (16, 48, 80 doubles for DP = 16, 32, 64: the four rows j .. j + 3
//               a wave reads at once fall on disjoint bank halves two by two, the rule of KMV_LDV; the A-stride tile of k_kmv_grad
//               overlaps them).  Per wave and column tile: (1 + CB) DP MFMA, against DP + R for k_kmv.
//   the shift   the second copy is written anyway, so it is written SHIFTED by the anchor m = the scaled first row of the row tile.
//               Out = 2 s_d ((sx_id - m_d) rho_ic - O_icd): the expanded form cancels in proportion to |sx - m| + |sy - m|, distances
//               from the anchor, where c has decayed -- not to the data's offset from the origin.  The d2 step keeps the unshifted copy.
// End of the walk: rho over the four lanes that share a row (fixed order), through LDS to the lanes that hold the row's outputs; each
// column group writes its own slice and k_kmv_sum adds the slices in ascending group order.  No atomics: two calls agree bit for bit,
// and in shared mode column c of Out is a function of column c of V alone.
// LDS (doubles): 2 x 64 (DP + 2) + 64 LDB + 64 LDVS (CB shared, 48 paired) + 128 norms + DP scales + DP anchor (DESIGN.md 9s has the table).
#pragma once
#include "agp_kmv.h"

namespace agp {

template <int DP>
constexpr int KMV_DX_LDB = DP == 16 ? 16 : DP + 16;  // = 16 (mod 32): rows j, j + 1 on disjoint bank halves
constexpr int KMV_DX_LDP = 48;                        // the paired V tile [j][i], i < 32: KMV_LDV<2>
constexpr int KMV_DX_MAXN = 32;                       // rows of X in paired mode
template <int DP, int CB, bool PAIRED>
constexpr size_t kmv_dx_smem_bytes() {
  return sizeof(double) * (size_t)(2 * TILE * (DP + 2) + TILE * KMV_DX_LDB<DP> + TILE * (PAIRED ? KMV_DX_LDP : CB) + 2 * TILE + 2 * DP);
}

// phi' alone, one exponential: kernel_dbase's expressions (the Materns on exp_nonpos, as kmv_phi_dphi)
template <int KIND>
__device__ __forceinline__ double kmv_dphi(double d2) {
  d2 = d2 > 0.0 ? d2 : 0.0;
  if constexpr (KIND == K_SQEXP) {
    return -0.5 * exp(-0.5 * d2);
  } else {
    const double r = sqrt(d2);
    if constexpr (KIND == K_MATERN52) {
      const double s5 = 2.23606797749978969641;
      return -(5.0 / 6.0) * (1.0 + s5 * r) * exp_nonpos(-s5 * r);
    } else {
      const double s3 = 1.73205080756887729353;
      return -1.5 * exp_nonpos(-s3 * r);
    }
  }
}

// grid = (column groups, row tiles, column blocks of CB right-hand sides; paired: 1).  Ysc / yng as in k_kmv.
// out: shared n x (r D), element [i][c D + d]; paired n x D; leading dimension ldo.  Group g writes at out + g * slice.
template <int KIND, int DP, int CB, bool PAIRED>
__global__ __launch_bounds__(NTHREADS, (DP == 64 || PAIRED) ? 1 : 2) void k_kmv_dx(
    const double* __restrict__ X, int64_t ldx, int64_t n, const double* __restrict__ Ysc, const double* __restrict__ yng, int64_t p,
    int64_t D, const double* __restrict__ scales, double variance, const double* __restrict__ V, int64_t ldv, int r,
    double* __restrict__ out, int64_t ldo, int64_t slice) {
  static_assert(!PAIRED || CB == 1, "paired mode has one right-hand side per row");
  constexpr int LDX = DP + 2, LDB = KMV_DX_LDB<DP>, W = PAIRED ? KMV_DX_MAXN : CB, LDVS = PAIRED ? KMV_DX_LDP : CB;
  constexpr int NK = DP / 4, NB = DP / 16, YQ = DP / 8, VQ = (TILE * W + NTHREADS - 1) / NTHREADS;
  extern __shared__ __attribute__((aligned(16))) unsigned char kmv_smem[];
  double* Xs = reinterpret_cast<double*>(kmv_smem);  // [64][LDX]
  double* Ys = Xs + TILE * LDX;                      // [64][LDX]  the d2 step's A operand, unshifted
  double* Yb = Ys + TILE * LDX;                      // [64][LDB]  the product's B operand, shifted by the anchor
  double* Vs = Yb + TILE * LDB;                      // [64][LDVS]
  double* xn = Vs + TILE * LDVS;                     // [64]
  double* yn = xn + TILE;                            // [64]
  double* sc = yn + TILE;                            // [DP]
  double* am = sc + DP;                              // [DP]  the anchor: the scaled first row of this row tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  const int c0 = PAIRED ? 0 : (int)blockIdx.z * CB;
  const int64_t nct = (p + TILE - 1) / TILE, base = nct / gridDim.x, rem = nct % gridDim.x;
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
      const int e = tid + NTHREADS * q, j = e / W, c = c0 + e % W;
      const int64_t gj = ct * TILE + j;
      vr[q] = (e < TILE * W && gj < p && c < r) ? V[gj * ldv + c] : 0.0;
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
  {  // four lanes per row, combined in a fixed order
    const int rr = tid >> 2, q4 = tid & 3;
    double s = 0.0;
    for (int d = q4; d < DP; d += 4) s += Xs[rr * LDX + d] * Xs[rr * LDX + d];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (q4 == 0) xn[rr] = s;
  }
  if (tid < DP) am[tid] = Xs[tid];  // (row i0 always exists)
  __syncthreads();
  const int il = wave * 16 + l15;  // this lane's row of the tile in the d2 and function steps
  double xb[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) xb[kk] = Xs[il * LDX + kk * 4 + l4];
  const double xnv = xn[il];
  const double close_thr = KMM_CLOSE<double>;
  // a thread writes the same pair of dimensions of every row it stages (NTHREADS is a multiple of DP / 2): its share of the anchor
  const double m0 = am[2 * (tid % (DP / 2))], m1 = am[2 * (tid % (DP / 2)) + 1];

  d4 o[CB][NB];
  double rho[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    rho[c] = 0.0;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
      for (int q = 0; q < 4; ++q) o[c][db][q] = 0.0;
  }

  for (int64_t ct = ct0; ct < ct1; ++ct) {
    if (ct != ct0) __syncthreads();  // the previous tile's products are done with Ys / Yb / Vs / yn
#pragma unroll
    for (int q = 0; q < YQ; ++q) {
      const int e = tid + NTHREADS * q, row = e / (DP / 2), v = e % (DP / 2);
      d2v t = yr[q];
      *reinterpret_cast<d2v*>(Ys + row * LDX + 2 * v) = t;
      t[0] -= m0;
      t[1] -= m1;
      *reinterpret_cast<d2v*>(Yb + row * LDB + 2 * v) = t;
    }
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q;
      if (e < TILE * W) Vs[(e / W) * LDVS + (e % W)] = vr[q];
    }
    if (tid < TILE) yn[tid] = ynr;
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products

    const double* pa = Ys + l15 * LDX + l4;
    const double* pb = Yb + l4 * LDB + l15;
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {  // (rolled for the reason given in k_kmv)
      d4 s[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[h][q] = 0.0;
      const double* pj = pa + jp * 32 * LDX;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double a = pj[h * 16 * LDX + kk * 4];
          lds_keep_apart();
          s[h] = Mfma<double>::mma(a, xb[kk], s[h]);
        }
      // function step: element q of s[h] is (row il, column 32 jp + 16 h + l4 + 4 q)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jp * 32 + h * 16 + l4 + 4 * q;
          const double s2 = xnv + yn[jl];
          double d2 = s2 - 2.0 * s[h][q];
          if (d2 < close_thr * s2) {  // (nearly) coincident points: direct differences, no cancellation
            double t = 0.0;
#pragma unroll 1
            for (int d = 0; d < DP; ++d) {
              const double df = Xs[il * LDX + d] - Ys[jl * LDX + d];
              t += df * df;
            }
            d2 = t;
          }
          s[h][q] = variance * kmv_dphi<KIND>(d2);
        }
      // product step: k-step 8 jp + 4 h + q takes c o v = s[h][q] V[j][c] as its A operand as it stands
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jp * 32 + h * 16 + l4 + 4 * q;
          double b[NB];
#pragma unroll
          for (int db = 0; db < NB; ++db) b[db] = pb[(jp * 32 + h * 16 + q * 4) * LDB + db * 16];
          lds_keep_apart();
#pragma unroll
          for (int c = 0; c < CB; ++c) {
            double v;
            if constexpr (PAIRED) v = il < KMV_DX_MAXN ? Vs[jl * LDVS + il] : 0.0;
            else v = Vs[jl * LDVS + c];
            const double a = s[h][q] * v;
            rho[c] += a;
#pragma unroll
            for (int db = 0; db < NB; ++db) o[c][db] = Mfma<double>::mma(a, b[db], o[c][db]);
          }
        }
    }
  }
  // ---- end of the walk: rho over the four lanes of a row, handed through LDS to the lanes that hold the row's outputs ----
  __syncthreads();  // every wave is done with Ys
  double* rs = Ys;  // [64][CB]
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    double t = rho[c];
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 32);
    if (l4 == 0) rs[il * CB + c] = t;
  }
  __syncthreads();
  double* dst = out + blockIdx.x * slice;
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // element q of o[c][db]: row wave * 16 + l4 + 4 q, dimension 16 db + l15
        const int row = wave * 16 + l4 + 4 * q, d = db * 16 + l15;
        const int64_t gi = i0 + row;
        if (gi < n && d < D && c0 + c < r) {
          const double val = 2.0 * sc[d] * ((Xs[row * LDX + d] - am[d]) * rs[row * CB + c] - o[c][db][q]);
          dst[gi * ldo + (PAIRED ? (int64_t)d : (int64_t)(c0 + c) * D + d)] = val;
        }
      }
}

}  // namespace agp
