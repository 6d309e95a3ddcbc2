// agp_kmv_f32.h -- the Float32 instance of the matrix-free kernel operator (agp_kmv.h):  Out = (K(X, Y) + diag_add [X is Y]) V  with
// both products on v_mfma_f32_16x16x4f32 and the kernel function on the hardware exp2, V and Out stored as Float32 OR Float64.
// Host side: agp_kmv_host.h (Kmv32Op, kmv32_prepare, kmv32_apply).  The work split is k_kmv's -- a 64-row tile of X per workgroup of
// four waves, wave w owns rows 16 w .. 16 w + 15, grid = (column groups, row tiles), register prefetch of the next tile, the kernel
// kind a template parameter, D <= 64, r <= 32 -- but this is not k_kmv with the type replaced.  Four things differ.
//
// (a) Register hand-over, f32 geometry.  The f32 accumulator map is row = 4 (lane >> 4) + q, column = lane & 15 (f64: row =
//     (lane >> 4) + 4 q).  With S' = Ys Xs' accumulator register q of block h holds K[i = lane & 15][j = 16 h + 4 (lane >> 4) + q].
//     Taken as the A operand as it stands (A: lane holds A[i = lane & 15][k = lane >> 4]), k-step (h, q) of the second product
//     contracts over the columns j = 16 h + q, 16 h + 4 + q, 16 h + 8 + q, 16 h + 12 + q, so its B operand is V row
//     16 h + 4 (lane >> 4) + q: the four rows a wave reads at once lie FOUR apart.  The V tile is staged as [j][c] with a row stride of
//     LDV = 20 (R = 16) or 36 (R = 32) floats: 4 LDV = 16 mod 64, so rows j, j + 4, j + 8, j + 12 start 16 banks apart and their 16
//     consecutive floats fall on the four disjoint quarters of the 64 banks -- one ds_read_b32 per operand, no conflict (LDV = R + 4 is
//     the smallest stride >= R with that property; R + 2, the f64 choice scaled, would put rows j and j + 8 on the same banks).  No K
//     tile in LDS, no barrier between the two products.  The output accumulators come out in the f32 row map too: element q of o[cb] is
//     row 16 w + 4 (lane >> 4) + q, column 16 cb + (lane & 15).
//     The d2 step reads its A operand (the Y tile) FOUR k-steps at a time: a dot product does not care in which order the input
//     dimensions are contracted, so k-step 4 g + e of the first product takes dimension 16 g + 4 (lane >> 4) + e from both sides, and a
//     lane's four A operands of group g are 16 consecutive bytes -- one ds_read_b128 per four MFMAs.  Row stride of the operand tiles
//     LDX = DP + 4 floats (20, 36, 68): 16-byte aligned rows, and LDX i mod 64 runs through the sixteen multiples of 4 for i = 0 .. 15,
//     so the sixteen rows of a read land on sixteen disjoint 4-bank groups.
// (b) No Float32 chain over N.  The second product runs in Float32 MFMA accumulators for a WINDOW of KMV32_F = 2 column tiles (128
//     terms); then the window is added into Float64 registers (4 R / 16 conversions and adds per lane) and the accumulators are
//     cleared.  F = 2: the window's worst-case error is gamma32_{128}, about 8e-6 relative to sum_j |K_ij V_jc| -- the level of the
//     kernel values' own budget -- and the flush is 16 VALU operations per 2 x (4 DP / 4 + 16 R / 16) MFMAs, under 2 % of the issue
//     slots at D = 32, r = 32.  What a column group writes is the Float64 sums; k_kmv32_sum adds the slices in ascending group order.
//     No atomics; two calls agree bit for bit; column c of Out depends on column c of V alone.
//     diag_add is NOT folded into the Float32 diagonal value (variance + sigma2 rounded to Float32 would move sigma2 by up to
//     2^-24 variance): group 0 adds diag_add V[i][c] to its Float64 sums with one FMA.  The diagonal VALUE is still exact: d2 = 0.
// (c) Both sides arrive prepared (k_kmv32_prep): centred by the per-dimension mean of X (k_kmv32_mean, a reduction of fixed order),
//     scaled, rounded to Float32 ONCE -- subtraction and scaling in Float64 whatever the input type --, rows padded to tiles, with
//     their squared norms (summed in Float64 from the rounded values, rounded once).  The kernels are stationary, so the shift changes
//     nothing but the size of |sx|^2 + |sy|^2, which is what the KMM_CLOSE<float> = 3e-2 repair and the GEMM form's error scale with:
//     on data at 10 + U[0, 1) every pair would otherwise take the divergent repair loop.  The repair itself stays, by direct
//     differences from the tiles in LDS, and so do the exact diagonal and exact duplicates (equal rows are prepared to equal bits).
// (d) One instance serves both storage types: vf32 / of32 are wave-uniform flags at the global loads of V and the stores of Out;
//     everything between is the same code.  4 kinds x 3 DP x 2 RB = 24 instances of k_kmv32, as many as k_kmv.  Every workgroup
//     streams all of V, so a caller with a Float64 V and room for n x r floats (the solver handle) has it rounded once per product
//     by k_kmv32_stage and the workgroups read half the bytes: the same rounding, the same bits.
// LDS (floats): 2 x 64 (DP + 4) operand tiles + 64 LDV for V + 128 norms:
//   DP = 64, R = 32: 43.5 KB (three workgroups per CU in 160 KB; f64: 93.7 KB, one); DP = 32, R = 32: 27.5 KB (five; f64 60.7 KB, two);
//   DP = 16, R = 16: 15.5 KB.  Registers decide the occupancy, not LDS: see DESIGN.md 9r.
#pragma once
#include "agp_kmv.h"

namespace agp {

constexpr int KMV32_F = 2;  // column tiles per Float32 accumulation window
template <int RB>
constexpr int KMV32_LDV = RB == 1 ? 20 : 36;
template <int DP, int RB>
constexpr size_t kmv32_smem_bytes() {
  return sizeof(float) * (size_t)(2 * TILE * (DP + 4) + TILE * KMV32_LDV<RB> + 2 * TILE);
}

// mean[d] = (1 / n) sum_i X[i][d] in Float64: one workgroup per dimension, 256 strided partial sums, a tree of fixed shape
template <typename TI>
__global__ __launch_bounds__(256) void k_kmv32_mean(const TI* __restrict__ X, int64_t ldx, int64_t n, double* __restrict__ mean) {
  __shared__ double red[256];
  const int tid = threadIdx.x, d = blockIdx.x;
  double s = 0.0;
  for (int64_t i = tid; i < n; i += 256) s += (double)X[i * ldx + d];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) mean[d] = red[0] / (double)n;
}

// Ysc[j][d] = float((Y[j][d] - mean[d]) * scales[d]) (rows padded to a multiple of 64 and columns to DP with zeros) and
// yn[j] = float(sum_d Ysc[j][d]^2), the sum in Float64.  One wave per row.
template <typename TI>
__global__ __launch_bounds__(256) void k_kmv32_prep(const TI* __restrict__ Y, int64_t ldy, int64_t p, int64_t p_pad, int64_t D, int DP,
                                                    const double* __restrict__ mean, const double* __restrict__ scales,
                                                    float* __restrict__ Ysc, float* __restrict__ yn) {
  const int64_t row = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= p_pad) return;
  float v = 0.0f;
  if (lane < DP) {
    if (row < p && lane < D) v = (float)(((double)Y[row * ldy + lane] - mean[lane]) * scales[lane]);
    Ysc[row * DP + lane] = v;
  }
  double s = (double)v * (double)v;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) yn[row] = (float)s;
}

// grid = (column groups, row tiles).  Xsc / xng and Ysc / yng: k_kmv32_prep's output with row width DP, rows padded to a multiple of
// 64 (the symmetric form passes the same arrays twice).  V: p x r (ldv), float if vf32 else double.  out: n x r with leading dimension
// ldo; group g writes at element offset g * slice (slice = 0 with one group: straight into the result), float if of32 else double
// (the slices of several groups are always double).  Vdiag (nullable, ldvd): the unrounded V when V itself is k_kmv32_stage's copy.
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, 2) void k_kmv32(const float* __restrict__ Xsc, const float* __restrict__ xng, int64_t n,
                                                      const float* __restrict__ Ysc, const float* __restrict__ yng, int64_t p,
                                                      float variance, int sym, double diag_add, const void* __restrict__ V,
                                                      int64_t ldv, int vf32, int r, void* __restrict__ out, int64_t ldo, int64_t slice,
                                                      int of32, const double* __restrict__ Vdiag, int64_t ldvd) {
  constexpr int LDX = DP + 4, LDV = KMV32_LDV<RB>, NG = DP / 16, VQ = 4 * RB, R = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char kmv32_smem[];
  float* Xs = reinterpret_cast<float*>(kmv32_smem);  // [64][LDX]
  float* Ys = Xs + TILE * LDX;                       // [64][LDX]
  float* Vs = Ys + TILE * LDX;                       // [64][LDV]
  float* xn = Vs + TILE * LDV;                       // [64]
  float* yn = xn + TILE;                             // [64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  // this group's column tiles: nct tiles over gridDim.x groups, the first nct % groups take one more
  const int64_t nct = (p + TILE - 1) / TILE, base = nct / gridDim.x, rem = nct % gridDim.x;
  const int64_t ct0 = blockIdx.x * base + ((int64_t)blockIdx.x < rem ? blockIdx.x : rem);
  const int64_t ct1 = ct0 + base + ((int64_t)blockIdx.x < rem ? 1 : 0);
  const float* Vf = static_cast<const float*>(V);
  const double* Vd = static_cast<const double*>(V);

  f4 yr[NG];
  float vr[VQ], ynr = 0.0f;
  auto fetch = [&](int64_t ct) {
    const float* src = Ysc + ct * TILE * DP;
#pragma unroll
    for (int q = 0; q < NG; ++q) yr[q] = *reinterpret_cast<const f4*>(src + (int64_t)(tid + NTHREADS * q) * 4);
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = ct * TILE + j;
      float v = 0.0f;
      if (gj < p && c < r) v = vf32 ? Vf[gj * ldv + c] : (float)Vd[gj * ldv + c];
      vr[q] = v;
    }
    if (tid < TILE) ynr = yng[ct * TILE + tid];
  };
  if (ct0 < ct1) fetch(ct0);

  // the X tile and its norms, ready-made: once per workgroup
  {
    const float* src = Xsc + i0 * DP;
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const int e = tid + NTHREADS * q, row = e / (DP / 4), v = e % (DP / 4);
      *reinterpret_cast<f4*>(Xs + row * LDX + 4 * v) = *reinterpret_cast<const f4*>(src + (int64_t)e * 4);
    }
    if (tid < TILE) xn[tid] = xng[i0 + tid];
  }
  __syncthreads();
  const int il = wave * 16 + l15;  // this lane's row of the tile in the d2 and function steps
  f4 xb[NG];                       // element e of xb[g]: dimension 16 g + 4 l4 + e of row il (k-step 4 g + e)
#pragma unroll
  for (int g = 0; g < NG; ++g) xb[g] = *reinterpret_cast<const f4*>(Xs + il * LDX + g * 16 + l4 * 4);
  const float xnv = xn[il];
  const float close_thr = KMM_CLOSE<float>;

  f4 o[RB];      // the current window, Float32
  double od[RB][4];  // the sums over windows, Float64
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[cb][q] = 0.0f, od[cb][q] = 0.0;
  auto flush = [&]() {
#pragma unroll
    for (int cb = 0; cb < RB; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) od[cb][q] += (double)o[cb][q], o[cb][q] = 0.0f;
  };

  int win = 0;
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t j0 = ct * TILE;
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
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products

    // 32 columns of the tile at a time, in a loop that is not unrolled (k_kmv's reason: registers); two accumulators keep two
    // independent MFMA chains going in the d2 step, RB in the product step
    const float* pa = Ys + l15 * LDX + l4 * 4;
    const float* pv = Vs + (4 * l4) * LDV + l15;
    const int64_t dg = sym ? (i0 + il) - j0 : (int64_t)-1;  // the local column of the diagonal element of this row, if in this tile
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {
      // d2 step: S'[h] (16 columns of Y x this wave's 16 rows of X)
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
      // kernel function on the accumulators: element q of s[h] is (row il, column 32 jp + 16 h + 4 l4 + q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int jb = jp * 32 + h * 16 + 4 * l4;
        const f4 ynv = *reinterpret_cast<const f4*>(yn + jb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jb + q;
          const bool diag = (int64_t)jl == dg;
          const float s2 = xnv + ynv[q];
          float d2 = s2 - 2.0f * s[h][q];
          if (diag) {
            d2 = 0.0f;  // the point against itself
          } else if (d2 < close_thr * s2) {  // (nearly) coincident points: direct differences, no cancellation
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
      // product step: k-step (h, q) takes s[h][q] as its A operand as it stands; B is V row 32 jp + 16 h + 4 l4 + q
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
    if (++win == KMV32_F) {
      flush();
      win = 0;
    }
  }
  if (win) flush();
  // element q of od[cb]: row wave * 16 + 4 l4 + q, column 16 cb + l15
  float* dstf = static_cast<float*>(out) + blockIdx.x * slice;
  double* dstd = static_cast<double*>(out) + blockIdx.x * slice;
  const bool add_diag = sym && blockIdx.x == 0 && diag_add != 0.0;
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t gi = i0 + wave * 16 + 4 * l4 + q;
      const int c = cb * 16 + l15;
      if (gi < n && c < r) {
        double val = od[cb][q];
        if (add_diag)
          val = __builtin_fma(diag_add, Vdiag ? Vdiag[gi * ldvd + c] : vf32 ? (double)Vf[gi * ldv + c] : Vd[gi * ldv + c], val);
        if (of32) dstf[gi * ldo + c] = (float)val;
        else dstd[gi * ldo + c] = val;
      }
    }
}

// Vs[i][c] (n x r, dense) = float(V[i][c]): a Float64 V rounded once per product instead of once per workgroup that streams it
__global__ __launch_bounds__(256) void k_kmv32_stage(const double* __restrict__ V, int64_t ldv, int64_t n, int r, float* __restrict__ Vs) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e < n * r) Vs[e] = (float)V[(e / r) * ldv + (e % r)];
}

// Out[i][c] = sum_g ws[g][i][c], ascending g (slices are n x r doubles, dense); Out float if of32 else double
__global__ __launch_bounds__(256) void k_kmv32_sum(const double* __restrict__ ws, int groups, int64_t n, int r, void* __restrict__ out,
                                                   int64_t ldo, int of32) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x, tot = n * r;
  if (e >= tot) return;
  double s = ws[e];
  for (int g = 1; g < groups; ++g) s += ws[g * tot + e];
  if (of32) static_cast<float*>(out)[(e / r) * ldo + (e % r)] = (float)s;
  else static_cast<double*>(out)[(e / r) * ldo + (e % r)] = s;
}

}  // namespace agp
