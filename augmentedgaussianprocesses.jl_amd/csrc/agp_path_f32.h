// agp_path_f32.h -- the Float32 instance of the fused path-evaluation operator (agp_path.h; host side: agp_path_host.h, path32_*):
//   Out[i][c] = sum_{j < L} amp cos(omega_j . (s o x_i) + phase_j) W[j][c]  +  sum_{r < N} variance base(d2(x_i, X_r)) V[r][c]
// with both products of both segments on v_mfma_f32_16x16x4f32, Out stored as Float32 (or as Float64 slices of a column group).  It is
// to k_path what k_kmv32 (agp_kmv_f32.h) is to k_kmv: the work split of k_path -- one workgroup of four waves owns 64 rows of x and
// walks ONE concatenated list of column tiles, ceil(L / 64) feature tiles, then ceil(N / 64) training tiles; column groups split that
// list by k_kmv's rule, each group writes its own slice of Float64 sums and k_kmv32_sum adds the slices in ascending order, no
// atomics -- in k_kmv32's geometry:
// (a) the f32 register hand-over.  With S' = T Xs' (T the tile: 64 rows of Omega, or of the training points) accumulator register q of
//     block h holds (x row lane & 15, tile row 16 h + 4 (lane >> 4) + q) and is the A operand of k-step (h, q) of the second product as
//     it stands; its B operand is row 16 h + 4 (lane >> 4) + q of the W / V tile, staged [j][c] with row stride KMV32_LDV so that rows
//     four apart fall on disjoint bank quarters.  Operand tiles have row stride DP + 4 floats and are read with one ds_read_b128 per
//     four k-steps (k-step 4 g + e contracts dimension 16 g + 4 (lane >> 4) + e on both sides).  No tile of Phi or K in LDS, no barrier
//     between the two products.
// (b) a feature tile is a kernel tile with another function on the accumulators: amp cosf(S' + phase'_j), where the kernel tile has
//     variance base(|sx|^2 + |sy|^2 - 2 S') with the KMM_CLOSE<float> repair by direct differences from the tiles in LDS.  The segments
//     are two loops over one body whose segment is a compile-time parameter; the register prefetch of the next tile crosses the seam
//     (it picks Omega / phase' / W or the training rows / norms / V by the tile's index, which is uniform).
// (c) no Float32 chain longer than a window: the Float32 accumulators of the second product run for KMV32_F = 2 tiles (128 terms) and
//     are then added into Float64 registers.  The window counter runs through the seam (a window may hold one feature tile and one
//     training tile) and starts at 0 with the column group.
// (d) centring, which is what is new here.  Both sides are centred by m, the per-dimension mean of the SCALED training rows
//     (k_kmv32_mean, Float64, fixed order).  Training rows: float(sX[r][d] - m[d]) from the snapshot's Float64 scaled rows
//     (k_kmv32_prep); test rows: the prologue forms fl64(x[i][d] s[d]) - m[d] in Float64 -- the product rounded on its own, NOT fused
//     with the subtraction, so a test point that equals a training point is prepared to the same bits -- and rounds once.  The kernels
//     are stationary: the shift changes nothing but the size of |sx|^2 + |sy|^2, which keeps the repair rare on data away from the
//     origin.  The features are not stationary, so the shift is compensated in the phase (k_path32_prep):
//       phase'_j = phase_j + omega_j . m , in Float64, reduced to [-pi, pi) in Float64, rounded to Float32 once,
//     and the Float32 argument is omega_j . (s o x_i - m) + phase'_j: its rounding error scales with the spread of the data about the
//     training mean and with |phase'_j| <= pi, not with the offset of the data.
// cos: the full-range Float32 cosf (argument reduction included), the counterpart of the cos k_path calls; NOT the hardware v_cos_f32.
// Rows of a partially filled last tile of either segment fetch W (V) as 0; the padded Omega rows and phases are 0, so they add
// amp cos(0) * 0 = 0 exactly.  Duplicates: equal rows have equal bits, the repair gives d2 = 0 and the value is the variance.
// LDS is k_kmv32's (kmv32_smem_bytes): two operand tiles, the W / V tile, 64 norms of x and 64 phases or norms of the tile:
//   DP = 64, R = 32: 43.5 KB; DP = 32, R = 32: 27.5 KB; DP = 16, R = 16: 15.5 KB.  4 kinds x 3 DP x 2 RB = 24 instances.
#pragma once
#include <type_traits>

#include "agp_kmv_f32.h"

namespace agp {

// Omega (L x D, dense) into the Float32 operand layout: Lp rows (a multiple of 64) of width DP, padding zero, each value rounded once;
// ph32[j] = float(reduce(phase_j + sum_d omega_jd m_d)), the sum in Float64 in the fixed order of a wave's shuffle tree, reduce(a) =
// a - 2 pi rint(a / 2 pi) in Float64; 0 on the padding.  One wave per row.
__global__ __launch_bounds__(256) void k_path32_prep(const double* __restrict__ omega, const double* __restrict__ phase, int64_t L,
                                                     int64_t Lp, int64_t D, int DP, const double* __restrict__ m,
                                                     float* __restrict__ om32, float* __restrict__ ph32) {
  const int64_t row = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Lp) return;
  double w = 0.0, s = 0.0;
  if (row < L && lane < D) w = omega[row * D + lane], s = w * m[lane];
  if (lane < DP) om32[row * DP + lane] = (float)w;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) {
    double a = 0.0;
    if (row < L) {
      constexpr double TWO_PI = 6.283185307179586476925;
      a = phase[row] + s;
      a -= TWO_PI * rint(a / TWO_PI);
    }
    ph32[row] = (float)a;
  }
}

// float(fl64(x s) - m): the product is rounded before the subtraction, as the training side's scaled rows were
__device__ __forceinline__ float path32_centre(double x, double s, double m) {
#pragma clang fp contract(off)
  const double t = x * s;
  return (float)(t - m);
}

// grid = (column groups, row tiles).  X: the test points as given (n x D, ldx), scales and m: D doubles.  Om / ph: k_path32_prep's output
// (L features); Ysc / yng: k_kmv32_prep's output for the p training points, row width DP, rows padded to a multiple of 64.  W: L x r
// (ldw), V: p x r (ldv), Float32.  out: n x r with leading dimension ldo, float if of32 else double; group g writes at element offset
// g * slice (slice = 0 with one group: straight into the result; the slices of several groups are always double).  A segment with no
// rows is never dereferenced.
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, 2) void k_path32(
    const double* __restrict__ X, int64_t ldx, int64_t n, int64_t D, const double* __restrict__ scales, const double* __restrict__ m,
    const float* __restrict__ Om, const float* __restrict__ ph, int64_t L, float amp, const float* __restrict__ W, int64_t ldw,
    const float* __restrict__ Ysc, const float* __restrict__ yng, int64_t p, float variance, const float* __restrict__ V, int64_t ldv,
    int r, void* __restrict__ out, int64_t ldo, int64_t slice, int of32) {
  constexpr int LDX = DP + 4, LDV = KMV32_LDV<RB>, NG = DP / 16, VQ = 4 * RB, R = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char path32_smem[];
  float* Xs = reinterpret_cast<float*>(path32_smem);  // [64][LDX]
  float* Ys = Xs + TILE * LDX;                        // [64][LDX]: a tile of Omega, or of the centred training points
  float* Vs = Ys + TILE * LDX;                        // [64][LDV]: the tile's rows of W, or of V
  float* xn = Vs + TILE * LDV;                        // [64]
  float* yn = xn + TILE;                              // [64]: the tile's phases, or squared norms
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  // the concatenated list: nft feature tiles, then the training tiles; this group's share by k_kmv's rule
  const int64_t nft = (L + TILE - 1) / TILE, nct = nft + (p + TILE - 1) / TILE;
  const int64_t base = nct / gridDim.x, rem = nct % gridDim.x;
  const int64_t ct0 = blockIdx.x * base + ((int64_t)blockIdx.x < rem ? blockIdx.x : rem);
  const int64_t ct1 = ct0 + base + ((int64_t)blockIdx.x < rem ? 1 : 0);

  f4 yr[NG];
  float vr[VQ], ynr = 0.0f;
  auto fetch = [&](int64_t ct) {
    const bool feat = ct < nft;  // uniform
    const int64_t lt = feat ? ct : ct - nft, rows = feat ? L : p, ldb = feat ? ldw : ldv;
    const float* src = (feat ? Om : Ysc) + lt * TILE * DP;
    const float* B = feat ? W : V;
#pragma unroll
    for (int q = 0; q < NG; ++q) yr[q] = *reinterpret_cast<const f4*>(src + (int64_t)(tid + NTHREADS * q) * 4);
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = lt * TILE + j;
      vr[q] = (gj < rows && c < r) ? B[gj * ldb + c] : 0.0f;
    }
    if (tid < TILE) ynr = (feat ? ph : yng)[lt * TILE + tid];
  };
  if (ct0 < ct1) fetch(ct0);

  // the X tile: scaled and centred in Float64, rounded once; its squared norms summed in Float64 from the rounded values
  for (int e = tid; e < TILE * DP; e += NTHREADS) {
    const int rr = e / DP, d = e % DP;
    const int64_t gr = i0 + rr;
    Xs[rr * LDX + d] = (gr < n && d < D) ? path32_centre(X[gr * ldx + d], scales[d], m[d]) : 0.0f;
  }
  __syncthreads();
  {  // four lanes per row, combined in a fixed order
    const int rr = tid >> 2, q4 = tid & 3;
    double s = 0.0;
    for (int d = q4; d < DP; d += 4) s += (double)Xs[rr * LDX + d] * (double)Xs[rr * LDX + d];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (q4 == 0) xn[rr] = (float)s;
  }
  __syncthreads();
  const int il = wave * 16 + l15;  // this lane's row of the tile in the first product and the function step
  f4 xb[NG];                       // element e of xb[g]: dimension 16 g + 4 l4 + e of row il (k-step 4 g + e)
#pragma unroll
  for (int g = 0; g < NG; ++g) xb[g] = *reinterpret_cast<const f4*>(Xs + il * LDX + g * 16 + l4 * 4);
  const float xnv = xn[il];
  const float close_thr = KMM_CLOSE<float>;

  f4 o[RB];          // the current window, Float32
  double od[RB][4];  // the sums over windows, Float64
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[cb][q] = 0.0f, od[cb][q] = 0.0;
  int win = 0;  // tiles in the current window; it runs through the seam

  // one tile of the list; FEAT (std::true_type / std::false_type) selects the function on the accumulators
  auto tile = [&](int64_t ct, auto FEAT) {
    constexpr bool feat = decltype(FEAT)::value;
    if (ct != ct0) __syncthreads();  // the previous tile's products are done with Ys / Vs / yn
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const int e = tid + NTHREADS * q, row = e / (DP / 4), v = e % (DP / 4);
      *reinterpret_cast<f4*>(Ys + row * LDX + 4 * v) = yr[q];
    }
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q;
      Vs[(e / R) * LDV + (e % R)] = vr[q];
    }
    if (tid < TILE) yn[tid] = ynr;
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products (the first training tile under the last feature tile)

    const float* pa = Ys + l15 * LDX + l4 * 4;
    const float* pv = Vs + (4 * l4) * LDV + l15;
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {
      // first product: S'[h] (16 rows of the tile x this wave's 16 rows of x)
      f4 s[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[h][q] = 0.0f;
      const float* pj = pa + jp * 32 * LDX;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f4 a[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) a[h] = *reinterpret_cast<const f4*>(pj + h * 16 * LDX + g * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int h = 0; h < 2; ++h) s[h] = Mfma<float>::mma(a[h][e], xb[g][e], s[h]);
      }
      // the function on the accumulators: element q of s[h] is (row il, tile row 32 jp + 16 h + 4 l4 + q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int jb = jp * 32 + h * 16 + 4 * l4;
        const f4 ynv = *reinterpret_cast<const f4*>(yn + jb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if constexpr (feat) {
            s[h][q] = amp * cosf(s[h][q] + ynv[q]);
          } else {
            const int jl = jb + q;
            const float s2 = xnv + ynv[q];
            float d2 = s2 - 2.0f * s[h][q];
            if (d2 < close_thr * s2) {  // (nearly) coincident points: direct differences, no cancellation
              float t = 0.0f;
#pragma unroll 1
              for (int d = 0; d < DP; ++d) {
                const float df = Xs[il * LDX + d] - Ys[jl * LDX + d];
                t += df * df;
              }
              d2 = t;
            }
            s[h][q] = variance * kernel_base<float>(KIND, d2);
          }
        }
      }
      // second product: k-step (h, q) takes s[h][q] as its A operand as it stands; B is row 32 jp + 16 h + 4 l4 + q of the W / V tile
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int cb = 0; cb < RB; ++cb) {
            const float b = pv[(jp * 32 + h * 16 + q) * LDV + cb * 16];
            lds_keep_apart();
            o[cb] = Mfma<float>::mma(s[h][q], b, o[cb]);
          }
    }
    if (++win == KMV32_F) {  // the window is full: into the Float64 sums
#pragma unroll
      for (int cb = 0; cb < RB; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) od[cb][q] += (double)o[cb][q], o[cb][q] = 0.0f;
      win = 0;
    }
  };
  const int64_t fe = ct1 < nft ? ct1 : nft;  // the end of this group's feature tiles
#pragma unroll 1
  for (int64_t ct = ct0; ct < fe; ++ct) tile(ct, std::true_type{});
#pragma unroll 1
  for (int64_t ct = ct0 > nft ? ct0 : nft; ct < ct1; ++ct) tile(ct, std::false_type{});
  if (win) {  // a last window of one tile
#pragma unroll
    for (int cb = 0; cb < RB; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) od[cb][q] += (double)o[cb][q];
  }

  // element q of od[cb]: row wave * 16 + 4 l4 + q, column 16 cb + l15
  float* dstf = static_cast<float*>(out) + blockIdx.x * slice;
  double* dstd = static_cast<double*>(out) + blockIdx.x * slice;
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t gi = i0 + wave * 16 + 4 * l4 + q;
      const int c = cb * 16 + l15;
      if (gi < n && c < r) {
        if (of32) dstf[gi * ldo + c] = (float)od[cb][q];
        else dstd[gi * ldo + c] = od[cb][q];
      }
    }
}

}  // namespace agp
