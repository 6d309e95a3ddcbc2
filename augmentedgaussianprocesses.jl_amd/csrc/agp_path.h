// agp_path.h -- the fused path-evaluation operator of the matrix-free pathwise draw (IterativeGP; host side: agp_path_host.h):
//   Out[i][c] = sum_{j < L} amp cos(omega_j . (s o x_i) + phase_j) W[j][c]  +  sum_{r < N} variance base(d2(x_i, X_r)) V[r][c]
// for a block of up to 32 columns in ONE launch: neither Phi(x) (n x L) nor K(x, X) (n x N) reaches memory.  Float64, D <= 64.
// Either segment may be empty: L > 0, N = 0 is the draw's Phi(X) W; both non-empty is an evaluation of the paths.
//
// k_path takes k_kmv's work split (agp_kmv.h).  One workgroup (4 waves) owns a 64-row tile of x, scaled once, the wave's 16 rows
// resident in registers as the B operand of the first product.  It walks ONE concatenated list of column tiles -- the feature tiles
// first, then the training tiles -- and keeps the 16 x R output accumulators in registers across both segments.  A feature tile is a
// kernel tile with another function on the accumulators:
//   first product   S' = Omega_tile Xs' on v_mfma_f64_16x16x4 (transposed, as k_kmv's cross term): the 64 Omega rows sit in the Y
//                   tile's LDS slot in the same prepared layout (row width DP, zero padded), phase_j where the column norms sit
//   function        amp cos(S' + phase_j) on the accumulators -- the Float64 device cos k_pw_features calls, its argument summed
//                   over d in the MFMA's order -- in place of variance base(|sx|^2 + |sy|^2 - 2 S') with the KMM_CLOSE repair
//   second product  Out += tile Wtile: the register hand-over of k_kmv (accumulator register q of S'[h] is the A operand of k-step
//                   4 h + q), W staged exactly like V.  No LDS round trip of the tile, no barrier between the two products.
// The segments are two loops over one body (the segment is a compile-time parameter of the body, so each loop carries one function
// only); the prefetch of the next tile runs across the seam: it picks Omega / phase / W or Xs / norms / V by the tile's index, which is
// uniform.  Rows of a partially filled last tile of either segment fetch W (V) as 0 and the tile's padded Omega rows and phases are
// 0, so they add amp cos(0) * 0 = 0 exactly.  Column groups split the CONCATENATED list (k_kmv's rule: the first nct % groups take one
// more tile), every group writes its own slice and k_kmv_sum adds the slices in ascending order: no atomics, two calls agree bit for
// bit, and column c of Out is a function of column c of W and V alone.  The kernel segment is k_kmv's general (non-symmetric) form:
// a test point that equals a training point is an ordinary input.
// Like k_kmv the 32-column loop is NOT unrolled: two accumulators, eight function values per lane in flight.
// LDS is k_kmv's budget (kmv_smem_bytes: Omega takes the Y tile's place, W the V tile's, phase the norms'):
//   DP = 64, R = 32: 93.7 KB (one workgroup per CU); DP = 32, R = 32: 60.7 KB (two); DP = 16, R = 16: 27.8 KB.
#pragma once
#include <type_traits>

#include "agp_kmv.h"

namespace agp {

// Omega (L x D, dense) into the prepared layout of k_scale_rows' tiles: Lp rows (a multiple of 64) of width DP, padding zero.  One
// lane per element of the tiles.
__global__ __launch_bounds__(256) void k_path_prep(const double* __restrict__ omega, int64_t L, int64_t Lp, int64_t D, int DP,
                                                   double* __restrict__ omt) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= Lp * DP) return;
  const int64_t j = e / DP, d = e % DP;
  omt[e] = (j < L && d < D) ? omega[j * D + d] : 0.0;
}

// R[i][s] = (b[i] - P[i][s]) - sigma E[i][s], in place in P (n x S, dense): the right-hand sides of the draw's solve
__global__ __launch_bounds__(256) void k_path_resid(int64_t n, int64_t S, const double* __restrict__ b, double sigma,
                                                    const double* __restrict__ E, double* __restrict__ P) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= n * S) return;
  P[e] = (b[e / S] - P[e]) - sigma * E[e];
}

// grid = (column groups, row tiles).  Om: k_path_prep's output (L features), ph: the phases padded with zeros to its rows; Ysc / yng:
// k_scale_rows' output for the training points (p of them) with row width DP.  W: L x r (ldw), V: p x r (ldv).  out: n x r with leading dimension ldo; group g writes at
// out + g * slice (slice = 0 with one group: straight into the result).  A segment with no rows is never dereferenced.
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, DP == 64 ? 1 : 2) void k_path(
    const double* __restrict__ X, int64_t ldx, int64_t n, const double* __restrict__ Om, const double* __restrict__ ph, int64_t L,
    double amp, const double* __restrict__ W, int64_t ldw, const double* __restrict__ Ysc, const double* __restrict__ yng, int64_t p,
    const double* __restrict__ V, int64_t ldv, int64_t D, const double* __restrict__ scales, double variance, int r,
    double* __restrict__ out, int64_t ldo, int64_t slice) {
  constexpr int LDX = DP + 2, LDV = KMV_LDV<RB>, NK = DP / 4, YQ = DP / 8, VQ = 4 * RB, R = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char path_smem[];
  double* Xs = reinterpret_cast<double*>(path_smem);  // [64][LDX]
  double* Ys = Xs + TILE * LDX;                       // [64][LDX]: a tile of Omega, or of the scaled training points
  double* Vs = Ys + TILE * LDX;                       // [64][LDV]: the tile's rows of W, or of V
  double* xn = Vs + TILE * LDV;                       // [64]
  double* yn = xn + TILE;                             // [64]: the tile's phases, or squared norms
  double* sc = yn + TILE;                             // [DP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  // the concatenated list: nft feature tiles, then the training tiles; this group's share by k_kmv's rule
  const int64_t nft = (L + TILE - 1) / TILE, nct = nft + (p + TILE - 1) / TILE;
  const int64_t base = nct / gridDim.x, rem = nct % gridDim.x;
  const int64_t ct0 = blockIdx.x * base + ((int64_t)blockIdx.x < rem ? blockIdx.x : rem);
  const int64_t ct1 = ct0 + base + ((int64_t)blockIdx.x < rem ? 1 : 0);

  d2v yr[YQ];
  double vr[VQ], ynr = 0.0;
  auto fetch = [&](int64_t ct) {
    const bool feat = ct < nft;  // uniform
    const int64_t lt = feat ? ct : ct - nft, rows = feat ? L : p, ldb = feat ? ldw : ldv;
    const double* src = (feat ? Om : Ysc) + lt * TILE * DP;
    const double* B = feat ? W : V;
#pragma unroll
    for (int q = 0; q < YQ; ++q) yr[q] = *reinterpret_cast<const d2v*>(src + (int64_t)(tid + NTHREADS * q) * 2);
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = lt * TILE + j;
      vr[q] = (gj < rows && c < r) ? B[gj * ldb + c] : 0.0;
    }
    if (tid < TILE) ynr = (feat ? ph : yng)[lt * TILE + tid];
  };
  if (ct0 < ct1) fetch(ct0);

  // scales, X tile (scaled), its squared norms: once per workgroup
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
  __syncthreads();
  const int il = wave * 16 + l15;  // this lane's row of the tile in the first product and the function step
  double xb[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) xb[kk] = Xs[il * LDX + kk * 4 + l4];
  const double xnv = xn[il];
  const double close_thr = KMM_CLOSE<double>;

  d4 o[RB];
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[cb][q] = 0.0;

  // one tile of the list; FEAT (std::true_type / std::false_type) selects the function on the accumulators
  auto tile = [&](int64_t ct, auto FEAT) {
    constexpr bool feat = decltype(FEAT)::value;
    if (ct != ct0) __syncthreads();  // the previous tile's products are done with Ys / Vs / yn
#pragma unroll
    for (int q = 0; q < YQ; ++q) {
      const int e = tid + NTHREADS * q, row = e / (DP / 2), v = e % (DP / 2);
      *reinterpret_cast<d2v*>(Ys + row * LDX + 2 * v) = yr[q];
    }
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q;
      Vs[(e / R) * LDV + (e % R)] = vr[q];
    }
    if (tid < TILE) yn[tid] = ynr;
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products (the first training tile under the last feature tile)

    const double* pa = Ys + l15 * LDX + l4;
    const double* pv = Vs + l4 * LDV + l15;
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {
      // first product: S'[h] (16 rows of the tile x this wave's 16 rows of x)
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
      // the function on the accumulators: element q of s[h] is (row il, column 32 jp + 16 h + l4 + 4 q)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jp * 32 + h * 16 + l4 + 4 * q;
          if constexpr (feat) {
            s[h][q] = amp * cos(s[h][q] + yn[jl]);
          } else {
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
            s[h][q] = variance * kernel_base<double>(KIND, d2);
          }
        }
      // second product: k-step 8 jp + 4 h + q takes s[h][q] as its A operand as it stands
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int cb = 0; cb < RB; ++cb) {
            const double b = pv[(jp * 32 + h * 16 + q * 4) * LDV + cb * 16];
            lds_keep_apart();
            o[cb] = Mfma<double>::mma(s[h][q], b, o[cb]);
          }
    }
  };
  const int64_t fe = ct1 < nft ? ct1 : nft;  // the end of this group's feature tiles
#pragma unroll 1
  for (int64_t ct = ct0; ct < fe; ++ct) tile(ct, std::true_type{});
#pragma unroll 1
  for (int64_t ct = ct0 > nft ? ct0 : nft; ct < ct1; ++ct) tile(ct, std::false_type{});

  // element q of o[cb]: row wave * 16 + l4 + 4 q, column 16 cb + l15
  double* dst = out + blockIdx.x * slice;
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t gi = i0 + wave * 16 + l4 + 4 * q;
      const int c = cb * 16 + l15;
      if (gi < n && c < r) dst[gi * ldo + c] = o[cb][q];
    }
}

}  // namespace agp
