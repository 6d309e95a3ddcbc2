// agp_kmv_hd.h -- the matrix-free kernel operator for 65 .. 128 input dimensions: Out = (K(X, Y) + diag_add [X is Y]) V for a block of
// up to 32 right-hand sides (k_kmv_hd).  Float64, all four kernel kinds, symmetric and general.  Host side: agp_kmv_host.h (kmv_apply
// sends op.D > 64 here); D <= 64 stays on k_kmv (agp_kmv.h), whose slice sum k_kmv_sum serves both.
//
// Why not kmv_body at DP = 128: its two 64 x (DP + 2) operand tiles and the V tile take 159.7 KB of the 160 KB of a CU, and its
// prefetch holds the whole next Y tile in registers (64 VGPRs) -- one workgroup per CU and nothing to overlap with.  What k_kmv_hd keeps
// of it is what makes the results comparable: one workgroup of 4 waves owns 64 rows of X and walks the column tiles of its column
// group, wave w owns rows 16 w .. 16 w + 15; both products on v_mfma_f64_16x16x4, the transposed first product S' = Ys Xs' handing the
// finished kernel values to the second IN REGISTERS; d2 = |sx|^2 + |sy|^2 - 2 S' with the KMM_CLOSE<double> repair by direct
// differences; d2 = 0 and + diag_add on the diagonal of the symmetric form; 32 columns of the tile at a time in a loop that is not
// unrolled (the function step then has 8 values per lane in flight, not 16: no scratch); column groups write their own slices; no
// atomics, fixed summation orders, column c of Out a function of column c of V alone.
//
// What is new is how the dimensions move:
//   X side      never in LDS.  Lane (l15, l4) of wave w loads its DP / 4 operands X[16 w + l15][4 kk + l4] * sc[4 kk + l4] straight from
//               global memory, once per launch, and keeps them (24 or 32 doubles).  The row norm is the sum of their squares over kk,
//               combined over the four lanes of the row (lanes l15 + 16 l4) by two exchanges -- the order of k_kmv's four-lane sum.
//   Y side      streamed through LDS in UNITS of 32 rows x 32 dimensions (3 chunks at DP = 96, 4 at DP = 128), rows padded to
//               LDX = 32 + 2 so that the 32 lanes one pass of a ds_read_b64 serves (16 rows x 2 k-offsets) cover all 64
//               banks once.  The units of a tile run half by half: (columns 0 .. 31: chunk 0, 1, ..), (columns 32 .. 63: chunk 0, 1, ..).
//               The two S' accumulators of a half are carried across its chunks; after the last chunk come the function step and the
//               product step of that half, exactly k_kmv's.
//   pipeline    two unit buffers in LDS and one unit in registers.  At unit g, after its ONE barrier: the registers (unit g + 1,
//               loaded during unit g - 1) go to the other buffer, the loads of unit g + 2 are issued -- the next chunk, the next
//               half's or the next tile's first chunk alike --, then the MFMA chain of unit g runs on its buffer with those loads in
//               flight.  The V rows and norms of a tile are loaded into registers under its first unit and stored behind the barrier
//               of its second: every wave has then finished the last product of the old tile, and the first function and product
//               steps of the new one come after the barrier of its third unit (there are at least three chunks).  The V rows are
//               therefore never live across a function step.  Chunks of 64 dimensions at DP = 128 (two chunks, the V rows loaded a
//               half tile ahead and held across the function step) took all 256 registers and left the second-order kernels 48 and
//               136 bytes of scratch per lane at R = 32.
//   repair      has to see whole rows, and no whole row is ever in LDS: it reads the X row from global memory, scales it with the
//               same single multiply (contraction off, so that the value is the fragment's, bit for bit) and subtracts the row of the
//               prepared tiles Ysc.  A duplicate row therefore gives d2 = 0 exactly.  Rare, and the rows are in cache.
// LDS: 2 x 32 x 34 unit buffers + 64 LDV for V + 64 norms, doubles: 25.5 KB at R = 16, 41.5 KB at R = 32, for both widths.  Two workgroups
// per CU in every instance (launch bounds; LDS would allow three): 256 registers per lane, of which the X fragments take 48 or 64,
// the accumulators 8 + 8 RB, the unit in flight 8 and the V rows 8 RB; the compiler takes 184 .. 249, no scratch
// (profiles/r06_kernel_resources.txt).  A third workgroup would leave 170 registers: less than every instance but two needs.
#pragma once
#include "agp_kmv.h"

namespace agp {

constexpr int KMV_HD_MAXD = 128;  // input dimensions of k_kmv_hd (above KMV_MAXD)
template <int DP>
constexpr int KMV_HD_CH = 32;  // dimensions per chunk (DP / 32 = 3 or 4 chunks: the V hand-over below needs at least 3)
template <int DP, int RB>
constexpr size_t kmv_hd_smem_bytes() {
  return sizeof(double) * (size_t)(2 * 32 * (KMV_HD_CH<DP> + 2) + TILE * KMV_LDV<RB> + TILE);
}

// The arguments of k_kmv; Ysc / yng: k_scale_rows' output for Y with row width DP (96 or 128).  Dynamic LDS: kmv_hd_smem_bytes<DP, RB>().
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, 2) void k_kmv_hd(const double* __restrict__ X, int64_t ldx, int64_t n,
                                                        const double* __restrict__ Ysc, const double* __restrict__ yng, int64_t p,
                                                        int64_t D, const double* __restrict__ scales, double variance, int sym,
                                                        double diag_add, const double* __restrict__ V, int64_t ldv, int r,
                                                        double* __restrict__ out, int64_t ldo, int64_t slice) {
  static_assert(DP == 96 || DP == 128, "the padded widths above 64");
  static_assert(RB == 1 || RB == 2, "16 or 32 right-hand sides");
  static_assert(DP / KMV_HD_CH<DP> >= 3, "V is stored behind the barrier of unit 1 and read after that of unit 2");
  constexpr int CH = KMV_HD_CH<DP>, NC = DP / CH, NU = 2 * NC, LDX = CH + 2, LDV = KMV_LDV<RB>, NK = DP / 4, CK = CH / 4;
  constexpr int HR = 32;                           // rows of Y per unit: half a tile
  constexpr int YQ = HR * CH / 2 / NTHREADS;       // d2v per lane and unit
  constexpr int VQ = 4 * RB, R = 16 * RB, UB = HR * LDX;
  extern __shared__ __attribute__((aligned(16))) unsigned char kmv_hd_smem[];
  double* Yb = reinterpret_cast<double*>(kmv_hd_smem);  // [2][32][LDX]
  double* Vs = Yb + 2 * UB;                             // [64][LDV]
  double* yn = Vs + TILE * LDV;                         // [64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  // this group's column tiles, as in k_kmv
  const int64_t nct = (p + TILE - 1) / TILE, base = nct / gridDim.x, rem = nct % gridDim.x;
  const int64_t ct0 = blockIdx.x * base + ((int64_t)blockIdx.x < rem ? blockIdx.x : rem);
  const int64_t ct1 = ct0 + base + ((int64_t)blockIdx.x < rem ? 1 : 0);

  d2v yr[YQ];
  double vr[VQ], ynr = 0.0;
  auto fetch_unit = [&](int64_t ct, int u) {  // unit u of tile ct: rows 32 (u / NC) .., dimensions CH (u % NC) ..
    const double* src = Ysc + (ct * TILE + (u / NC) * HR) * DP + (u % NC) * CH;
#pragma unroll
    for (int q = 0; q < YQ; ++q) {
      const int e = tid + NTHREADS * q, row = e / (CH / 2), v = e % (CH / 2);
      yr[q] = *reinterpret_cast<const d2v*>(src + (int64_t)row * DP + 2 * v);
    }
  };
  auto store_unit = [&](double* dstb) {
#pragma unroll
    for (int q = 0; q < YQ; ++q) {
      const int e = tid + NTHREADS * q, row = e / (CH / 2), v = e % (CH / 2);
      *reinterpret_cast<d2v*>(dstb + row * LDX + 2 * v) = yr[q];
    }
  };
  auto fetch_v = [&](int64_t ct) {
#pragma unroll
    for (int q = 0; q < VQ; ++q) {
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = ct * TILE + j;
      vr[q] = (gj < p && c < r) ? V[gj * ldv + c] : 0.0;
    }
    if (tid < TILE) ynr = yng[ct * TILE + tid];
  };
  if (ct0 < ct1) fetch_unit(ct0, 0);

  // the wave's X fragments and this lane's row norm: once per launch, from global memory
  const int il = wave * 16 + l15;  // this lane's row of the tile
  const int64_t gr = i0 + il;
  double xb[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    const int d = kk * 4 + l4;
    xb[kk] = (gr < n && d < D) ? X[gr * ldx + d] * scales[d] : 0.0;
  }
  double xnv = 0.0;
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) xnv += xb[kk] * xb[kk];
  xnv += __shfl_xor(xnv, 16);
  xnv += __shfl_xor(xnv, 32);
  const double close_thr = KMM_CLOSE<double>;

  d4 o[RB];
#pragma unroll
  for (int cb = 0; cb < RB; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) o[cb][q] = 0.0;

  int par = 0;  // the buffer of the current unit
  if (ct0 < ct1) {
    store_unit(Yb);
    fetch_unit(ct0, 1);
  }
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t j0 = ct * TILE;
    const bool more = ct + 1 < ct1;
    const double* pv = Vs + l4 * LDV + l15;
    const int64_t dg = sym ? (i0 + il) - j0 : (int64_t)-1;  // the local column of the diagonal element of this row, if in this tile
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {
      d4 s[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[h][q] = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int u = jp * NC + c;
        __syncthreads();  // unit u is in its buffer; every wave is done with the other one (and, at u = 1, with the last tile's Vs / yn)
        if (u + 1 < NU || more) store_unit(Yb + (par ^ 1) * UB);
        if (u == 1) {
#pragma unroll
          for (int q = 0; q < VQ; ++q) {
            const int e = tid + NTHREADS * q;
            Vs[(e / R) * LDV + (e % R)] = vr[q];
          }
          if (tid < TILE) yn[tid] = ynr;
        }
        // in flight under this unit's MFMA chain: the unit after the next, and under the tile's first unit its V rows and norms
        if (u + 2 < NU) fetch_unit(ct, u + 2);
        else if (more) fetch_unit(ct + 1, u + 2 - NU);
        if (u == 0) fetch_v(ct);
        // d2 step, chunk c: S'[h] += (16 columns of Y) x (this wave's 16 rows of X) over CH dimensions
        const double* pj = Yb + par * UB + l15 * LDX + l4;
#pragma unroll
        for (int kk = 0; kk < CK; ++kk)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const double a = pj[h * 16 * LDX + kk * 4];
            lds_keep_apart();
            s[h] = Mfma<double>::mma(a, xb[c * CK + kk], s[h]);
          }
        par ^= 1;
      }
      // kernel function on the accumulators: element q of s[h] is (row il, column 32 jp + 16 h + l4 + 4 q)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jl = jp * 32 + h * 16 + l4 + 4 * q;
          const bool diag = (int64_t)jl == dg;
          const double s2 = xnv + yn[jl];
          double d2 = s2 - 2.0 * s[h][q];
          if (diag) {
            d2 = 0.0;  // the point against itself
          } else if (d2 < close_thr * s2 && gr < n) {  // (nearly) coincident points: direct differences of whole rows, from global memory
            const double* xrow = X + gr * ldx;
            const double* yrow = Ysc + (j0 + jl) * DP;
            double t = 0.0;
#pragma unroll 1
            for (int d = 0; d < (int)D; ++d) {
              double xs;
              {
#pragma clang fp contract(off)
                xs = xrow[d] * scales[d];  // the fragment's value: one multiply, never fused into the difference
              }
              const double df = xs - yrow[d];
              t += df * df;
            }
            d2 = t;
          }
          double val = variance * kernel_base<double>(KIND, d2);
          if (diag) val += diag_add;
          s[h][q] = val;
          if (q == 3) __builtin_amdgcn_sched_barrier(0);  // 4 values at a time, not all 8 interleaved: registers
        }
      // product step: k-step 8 jp + 4 h + q takes s[h][q] as its A operand as it stands
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
  }
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
