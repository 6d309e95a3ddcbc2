// agp_kmv.h -- the matrix-free kernel operator  Out = (K(X, Y) + diag_add [X is Y]) V  for a block of up to 32 right-hand sides
// (k_kmv, k_kmv_sum) and the vector kernels of the batched preconditioned CG that runs on it (k_cg_*).  Float64 only.
// Host side: agp_kmv_host.h.  K never reaches memory: N is limited by time, not by 8 N^2 bytes.
//
// k_kmv -- the flash-attention shape on a Gram matrix.  One workgroup (4 waves) owns a 64-row tile of X and walks the column tiles of
// one column group of Y; wave w owns rows 16 w .. 16 w + 15 against all 64 columns of a tile.
//   d2 step     S' = Ys Xs' on v_mfma_f64_16x16x4 -- the TRANSPOSED cross term: A operand = the Y tile (k_scale_rows' ready-made
//               rows) read from LDS with one ds_read_b64 per operand, B operand = the wave's 16 X rows, which never change and stay
//               in registers for the whole launch (DP / 4 doubles per lane).  32 columns (two accumulators) at a time.
//   function    d2 = |sx|^2 + |sy|^2 - 2 S', the KMM_CLOSE<T> repair by direct differences from the tiles in LDS, d2 = 0 on the
//               diagonal of the symmetric form, then variance * base(d2) (+ diag_add on the diagonal), KIND a template parameter --
//               all in the accumulator registers.
//   product     Out += Ktile Vtile on the same instruction.  Accumulator register r of S'[jb] holds K[i = lane & 15][j = 16 jb + 4 r +
//               (lane >> 4)]: exactly the A-operand layout of k-step 4 jb + r of the second product.  The finished tile is therefore
//               handed over IN REGISTERS -- no LDS round trip, no barrier between the two products, and the 33 KB a 64 x 66 K tile
//               would take in LDS buy a second workgroup per CU instead.  The B operand is the V tile, staged in LDS as [j][c] with a
//               row stride of 16 (R = 16) or 48 (R = 32) doubles: rows j, j + 1 land on disjoint bank halves, one ds_read_b64 each.
//   prefetch    the next tile's Y rows, norms and V rows are loaded into registers before the current tile's products start and go
//               to LDS behind them (one buffer, two barriers per tile).
// The 16 x R accumulators of a wave (R = r padded to 16) stay in registers across all column tiles of the group; with several groups
// every group writes its own n x r slice and k_kmv_sum adds the slices in ascending group order.  No atomics, fixed summation
// orders: two calls agree bit for bit, and column c of Out is a function of column c of V alone (an MFMA output element is a dot
// product of its own row and column).
// LDS (DP = D padded to 16, 32 or 64; doubles): 2 x 64 (DP + 2) operand tiles + 64 LDV for V + 128 norms + DP scales:
//   DP = 64, R = 32: 93.7 KB (one workgroup per CU); DP = 32, R = 32: 60.7 KB (two); DP = 16, R = 16: 27.8 KB.
// D > 64 is not served here (the operand tiles and X fragments are sized at compile time): 65 .. 128 dimensions have k_kmv_hd
// (agp_kmv_hd.h), which streams the dimensions through LDS in chunks.
#pragma once
#include "agp_cavi.h"
#include "agp_chol.h"  // lds_keep_apart

namespace agp {

constexpr int KMV_MAXD = 64;  // input dimensions
constexpr int KMV_MAXR = 32;  // right-hand sides per launch
// row stride of the V tile: R = 16 RB rounded up to 16 (mod 32), so rows j, j + 1 start half the banks apart -- 16 (RB = 1: one row per
// pass), 48 (RB = 2), and 48, 80, 112, 144 for the wide block's RB = 3, 4, 6, 8 (agp_kmv_wide.h)
template <int RB>
constexpr int KMV_LDV = RB == 1 ? 16 : (16 * RB) % 32 == 16 ? 16 * RB : 16 * RB + 16;
template <int DP, int RB>
constexpr size_t kmv_smem_bytes() {
  return sizeof(double) * (size_t)(2 * TILE * (DP + 2) + TILE * KMV_LDV<RB> + 2 * TILE + DP);
}

// grid = (column groups, row tiles).  Ysc / yng: k_scale_rows' output for Y with row width DP, rows padded to a multiple of 64.
// out: n x r with leading dimension ldo; group g writes at out + g * slice (slice = 0 with one group: straight into the result).
// kmv_body is the whole kernel: k_kmv (RB = 1, 2) and k_kmv_wide (agp_kmv_wide.h: RB = 3, 4, 6, 8) are this one body under their own
// launch bounds, so the two paths cannot drift apart and a column is the same chain of operations in both.
template <int KIND, int DP, int RB>
__device__ __forceinline__ void kmv_body(const double* __restrict__ X, int64_t ldx, int64_t n, const double* __restrict__ Ysc,
                                         const double* __restrict__ yng, int64_t p, int64_t D, const double* __restrict__ scales,
                                         double variance, int sym, double diag_add, const double* __restrict__ V, int64_t ldv, int r,
                                         double* __restrict__ out, int64_t ldo, int64_t slice) {
  constexpr int LDX = DP + 2, LDV = KMV_LDV<RB>, NK = DP / 4, YQ = DP / 8, VQ = 4 * RB, R = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char kmv_smem[];
  double* Xs = reinterpret_cast<double*>(kmv_smem);  // [64][LDX]
  double* Ys = Xs + TILE * LDX;                      // [64][LDX]
  double* Vs = Ys + TILE * LDX;                      // [64][LDV]
  double* xn = Vs + TILE * LDV;                      // [64]
  double* yn = xn + TILE;                            // [64]
  double* sc = yn + TILE;                            // [DP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int64_t i0 = blockIdx.y * (int64_t)TILE;
  // this group's column tiles: nct tiles over gridDim.x groups, the first nct % groups take one more
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
      const int e = tid + NTHREADS * q, j = e / R, c = e % R;
      const int64_t gj = ct * TILE + j;
      vr[q] = (gj < p && c < r) ? V[gj * ldv + c] : 0.0;
    }
    if (tid < TILE) ynr = yng[ct * TILE + tid];
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
  const int il = wave * 16 + l15;  // this lane's row of the tile in the d2 and function steps
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
      Vs[(e / R) * LDV + (e % R)] = vr[q];
    }
    if (tid < TILE) yn[tid] = ynr;
    __syncthreads();
    if (ct + 1 < ct1) fetch(ct + 1);  // in flight under this tile's products

    // The three steps on 32 columns of the tile at a time, in a loop that is NOT unrolled: with all 16 values of a lane in flight the
    // compiler interleaved 16 evaluations of the kernel function and ran out of registers (the first-order kernels carried up to
    // 192 bytes of scratch per lane); two accumulators keep two independent MFMA chains going.
    const double* pa = Ys + l15 * LDX + l4;
    const double* pv = Vs + l4 * LDV + l15;
    const int64_t dg = sym ? (i0 + il) - j0 : (int64_t)-1;  // the local column of the diagonal element of this row, if in this tile
#pragma unroll 1
    for (int jp = 0; jp < 2; ++jp) {
      // d2 step: S'[h] (16 columns of Y x this wave's 16 rows of X)
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
          } else if (d2 < close_thr * s2) {  // (nearly) coincident points: direct differences, no cancellation
            double t = 0.0;
#pragma unroll 1
            for (int d = 0; d < DP; ++d) {
              const double df = Xs[il * LDX + d] - Ys[jl * LDX + d];
              t += df * df;
            }
            d2 = t;
          }
          double val = variance * kernel_base<double>(KIND, d2);
          if (diag) val += diag_add;
          s[h][q] = val;
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
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, DP == 64 ? 1 : 2) void k_kmv(const double* __restrict__ X, int64_t ldx, int64_t n,
                                                                    const double* __restrict__ Ysc, const double* __restrict__ yng,
                                                                    int64_t p, int64_t D, const double* __restrict__ scales,
                                                                    double variance, int sym, double diag_add,
                                                                    const double* __restrict__ V, int64_t ldv, int r,
                                                                    double* __restrict__ out, int64_t ldo, int64_t slice) {
  kmv_body<KIND, DP, RB>(X, ldx, n, Ysc, yng, p, D, scales, variance, sym, diag_add, V, ldv, r, out, ldo, slice);
}

// Out[i][c] = sum_g ws[g][i][c], ascending g (slices are n x r, dense)
__global__ __launch_bounds__(256) void k_kmv_sum(const double* __restrict__ ws, int groups, int64_t n, int r,
                                                 double* __restrict__ out, int64_t ldo) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x, tot = n * r;
  if (e >= tot) return;
  double s = ws[e];
  for (int g = 1; g < groups; ++g) s += ws[g * tot + e];
  out[(e / r) * ldo + (e % r)] = s;
}

// ---------------------------------------------------------------------------------------------------
// Batched preconditioned CG: r <= 32 independent recurrences that share every operator product.  All vectors are n x 32 row-major
// (CG_LD), columns >= r zero.  Per-column scalars live in CgScal on the device, double-buffered by iteration parity: the workgroup
// that finishes an iteration's scalars writes buffer (it + 1) & 1 while the others still read buffer it & 1.
// A handle set to the block of 128 (agp_gp_cg_set_block) keeps its vectors n x 128 (`ld`) and runs the same kernels on a grid whose
// y index is the PANEL of 32 columns: panel q owns columns 32 q .. 32 q + 31, the CgScal pair sc[2 q], sc[2 q + 1] and its own partials
// (part + q nblk 32).  A column's recurrence reads nothing of another column, so it is the arithmetic of the block of 32 unchanged;
// with ld = 32 and one panel every index below is the one it was.
// Column dots are two-stage and of fixed order: every workgroup of 256 rows leaves one partial per column (rows in a fixed
// tree), and whoever needs the dot adds the partials in ascending workgroup order -- every workgroup for itself, same bits.
// A column is ACTIVE while it is neither converged nor broken down; an inactive column is skipped, not multiplied by zero: its
// x, r, z, p keep their bits whatever the other columns do and however long the solve runs on.
// ---------------------------------------------------------------------------------------------------
constexpr int CG_LD = 32;
constexpr int CG_ROWS = 256;  // rows per workgroup of the vector kernels (8 rows x 32 columns per pass)
struct CgScal {
  double rz[CG_LD];     // r . z
  double bb[CG_LD];     // |b|^2
  double rr[CG_LD];     // |r|^2 (recursive residual)
  int32_t active[CG_LD];
  int32_t conv[CG_LD];
  int32_t iters[CG_LD];
};

// sum over the rows of this workgroup of v (one value per thread; thread = (row & 7, column)); result valid for threadIdx.x < 32
__device__ __forceinline__ double cg_block_coldot(double v, double* red /* [256] */) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  double s = 0.0;
  if (tid < CG_LD)
#pragma unroll
    for (int q = 0; q < 8; ++q) s += red[q * CG_LD + tid];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double cg_sum_parts(const double* __restrict__ part, int64_t nblk, int c) {
  double s = 0.0;
  for (int64_t b = 0; b < nblk; ++b) s += part[b * CG_LD + c];
  return s;
}
// this workgroup's panel: its partials and its slot among them
__device__ __forceinline__ int64_t cg_part_base(int64_t nblk) { return (int64_t)blockIdx.y * nblk * CG_LD; }

// part[blk][c] = sum_{rows of blk} A[i][c] B[i][c]
__global__ __launch_bounds__(256) void k_cg_dot(const double* __restrict__ A, const double* __restrict__ B, int64_t n, int64_t ld,
                                                double* __restrict__ part) {
  __shared__ double red[256];
  const int tid = threadIdx.x, c = blockIdx.y * CG_LD + (tid & 31);
  const int64_t r0 = blockIdx.x * (int64_t)CG_ROWS;
  double s = 0.0;
  for (int q = tid >> 5; q < CG_ROWS; q += 8) {
    const int64_t i = r0 + q;
    if (i < n) s += A[i * ld + c] * B[i * ld + c];
  }
  s = cg_block_coldot(s, red);
  if (tid < CG_LD) part[cg_part_base(gridDim.x) + blockIdx.x * CG_LD + tid] = s;
}

// init != 0: x = 0, r = B (n x r, ldb; columns >= r zero).  Otherwise alpha = rz / (p . q) from the partials of k_cg_dot,
// x += alpha p, r -= alpha q on the active columns.  Both: part_rr[blk][c] = partial |r|^2, and Rt (nullable) = r transposed,
// [c][i] with leading dimension ldt (the A operand of the preconditioner's first GEMM).  coef (nullable): this iteration's row of the
// Lanczos table, [2][32]: workgroup 0 stores alpha per column (0 for a column that did not step); nothing else changes with it.
__global__ __launch_bounds__(256) void k_cg_update(int init, const double* __restrict__ B, int64_t ldb, int rcols, int64_t n,
                                                   int64_t nblk, const CgScal* __restrict__ sc, const double* __restrict__ part_pq,
                                                   const double* __restrict__ P, const double* __restrict__ Q,
                                                   double* __restrict__ Xv, double* __restrict__ Rv, double* __restrict__ Rt,
                                                   int64_t ldt, double* __restrict__ part_rr, double* __restrict__ coef,
                                                   int64_t ld) {
  __shared__ double red[256];
  const int tid = threadIdx.x, lc = tid & 31, c = blockIdx.y * CG_LD + lc;  // lc: the column within this panel's scalars and partials
  const int64_t r0 = blockIdx.x * (int64_t)CG_ROWS;
  sc += 2 * blockIdx.y;
  part_pq += cg_part_base(nblk);
  bool act = false;
  double alpha = 0.0;
  if (!init && sc->active[lc]) {
    const double pq = cg_sum_parts(part_pq, nblk, lc);
    act = pq > 0.0;  // (a breakdown is recorded by k_cg_direction, from the same sum)
    if (act) alpha = sc->rz[lc] / pq;
  }
  if (coef && blockIdx.x == 0 && tid < CG_LD) coef[c] = alpha;
  double s = 0.0;
  for (int q = tid >> 5; q < CG_ROWS; q += 8) {
    const int64_t i = r0 + q;
    if (i >= n) continue;
    double rv;
    if (init) {
      rv = c < rcols ? B[i * ldb + c] : 0.0;
      Xv[i * ld + c] = 0.0;
      Rv[i * ld + c] = rv;
    } else {
      rv = Rv[i * ld + c];
      if (act) {
        Xv[i * ld + c] = __builtin_fma(alpha, P[i * ld + c], Xv[i * ld + c]);
        rv = __builtin_fma(-alpha, Q[i * ld + c], rv);
        Rv[i * ld + c] = rv;
      }
    }
    if (Rt && (init || act)) Rt[c * ldt + i] = rv;
    s += rv * rv;
  }
  s = cg_block_coldot(s, red);
  if (tid < CG_LD) part_rr[cg_part_base(nblk) + blockIdx.x * CG_LD + tid] = s;
}

// z = (r - Zl) / sigma2 (Woodbury; Zl = L (sigma2 I + L'L)^-1 L' r, n x 64 with leading dimension ldz) and the partials of r . z
__global__ __launch_bounds__(256) void k_cg_precond(int64_t n, const double* __restrict__ Rv, const double* __restrict__ Zl,
                                                    int64_t ldz, double inv_sigma2, double* __restrict__ Z,
                                                    double* __restrict__ part_rz, int64_t ld) {
  __shared__ double red[256];
  const int tid = threadIdx.x, c = blockIdx.y * CG_LD + (tid & 31);
  const int64_t r0 = blockIdx.x * (int64_t)CG_ROWS;
  double s = 0.0;
  for (int q = tid >> 5; q < CG_ROWS; q += 8) {
    const int64_t i = r0 + q;
    if (i >= n) continue;
    const double rv = Rv[i * ld + c], z = (rv - Zl[i * ldz + c]) * inv_sigma2;
    Z[i * ld + c] = z;
    s += rv * z;
  }
  s = cg_block_coldot(s, red);
  if (tid < CG_LD) part_rz[cg_part_base(gridDim.x) + blockIdx.x * CG_LD + tid] = s;
}

// The end of an iteration (init != 0: of the set-up).  rz_new and |r|^2 from their partials; a column whose |r|^2 <= tol^2 |b|^2
// becomes inactive and counts as converged (a zero column of B at once, with zero iterations); one whose p . q or r . z is not
// positive breaks down: inactive, not converged.  Still active: p = z + (rz_new / rz) p.  Z == nullptr: no preconditioner, z = r and
// r . z = |r|^2.  Workgroup 0 writes the next scalars, and beta per column into coef[32 + c] (nullable; 0 where p was not updated).
__global__ __launch_bounds__(256) void k_cg_direction(int init, int64_t n, int64_t nblk, double tol2, const CgScal* __restrict__ sc,
                                                      CgScal* __restrict__ sc_next, const double* __restrict__ part_pq,
                                                      const double* __restrict__ part_rr, const double* __restrict__ part_rz,
                                                      const double* __restrict__ Rv, const double* __restrict__ Z,
                                                      double* __restrict__ P, double* __restrict__ coef, int64_t ld) {
  const int tid = threadIdx.x, lc = tid & 31;
  const int64_t r0 = blockIdx.x * (int64_t)CG_ROWS;
  sc += 2 * blockIdx.y, sc_next += 2 * blockIdx.y;
  part_pq += cg_part_base(nblk), part_rr += cg_part_base(nblk), part_rz += cg_part_base(nblk);
  const bool was = init ? true : sc->active[lc] != 0;
  double rr = init ? 0.0 : sc->rr[lc], rz = init ? 0.0 : sc->rz[lc], bb = init ? 0.0 : sc->bb[lc], beta = 0.0;
  bool act = false, conv = init ? false : sc->conv[lc] != 0, stepped = false;
  if (was) {
    stepped = init || cg_sum_parts(part_pq, nblk, lc) > 0.0;
    if (stepped) {
      rr = cg_sum_parts(part_rr, nblk, lc);
      const double rz_new = Z ? cg_sum_parts(part_rz, nblk, lc) : rr;
      if (init) bb = rr;
      conv = rr <= tol2 * bb;  // (bb = 0: a zero column, converged with x = 0)
      act = !conv && rz_new > 0.0;
      if (act && !init) beta = rz_new / rz;
      rz = rz_new;
    }
  }
  const int c = blockIdx.y * CG_LD + lc;
  if (act)
    for (int q = tid >> 5; q < CG_ROWS; q += 8) {
      const int64_t i = r0 + q;
      if (i >= n) continue;
      const double z = Z ? Z[i * ld + c] : Rv[i * ld + c];
      P[i * ld + c] = init ? z : __builtin_fma(beta, P[i * ld + c], z);
    }
  if (blockIdx.x == 0 && tid < CG_LD) {
    if (coef) coef[ld + c] = beta;
    sc_next->rz[lc] = rz;
    sc_next->bb[lc] = bb;
    sc_next->rr[lc] = rr;
    sc_next->active[lc] = act ? 1 : 0;
    sc_next->conv[lc] = conv ? 1 : 0;
    sc_next->iters[lc] = init ? 0 : sc->iters[lc] + ((was && stepped) ? 1 : 0);
  }
}

// out[i][c] (ldo) = A[i][c] (n x ld), c < r
__global__ __launch_bounds__(256) void k_cg_export(const double* __restrict__ A, int64_t n, int r, double* __restrict__ out,
                                                   int64_t ldo, int64_t ld) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x, i = e / ld;
  const int c = (int)(e % ld);
  if (i < n && c < r) out[i * ldo + c] = A[e];
}
// out[i][c] (ldo) = scale * A[i][c] (n x ld), c < r: the copy of the first preconditioned residual z0 = P^-1 b
__global__ __launch_bounds__(256) void k_cg_export_scaled(const double* __restrict__ A, int64_t n, int r, double scale,
                                                          double* __restrict__ out, int64_t ldo, int64_t ld) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x, i = e / ld;
  const int c = (int)(e % ld);
  if (i < n && c < r) out[i * ldo + c] = scale * A[e];
}
// probes z ~ N(0, L L' + sigma2 I): out[i][c] (ldo) = Zl[i][c] (= L eps1, n x 64 with leading dimension ldz; nullable) + sigma E[c][i],
// E the base normals, one row of length lde per probe with eps2 in its first n entries
__global__ __launch_bounds__(256) void k_cg_probe(int64_t n, int r, const double* __restrict__ Zl, int64_t ldz, double sigma,
                                                  const double* __restrict__ E, int64_t lde, double* __restrict__ out, int64_t ldo) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x, i = e / CG_LD;
  const int c = (int)(e % CG_LD);
  if (i < n && c < r) out[i * ldo + c] = __builtin_fma(sigma, E[c * lde + i], Zl ? Zl[i * ldz + c] : 0.0);
}
// a = 0 (a small kernel instead of a memset node, so that a solve may be captured into a graph)
__global__ __launch_bounds__(256) void k_cg_zero(double* __restrict__ a, int64_t cnt) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e < cnt) a[e] = 0.0;
}

}  // namespace agp
