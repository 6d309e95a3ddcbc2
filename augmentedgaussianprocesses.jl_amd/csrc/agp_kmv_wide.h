// agp_kmv_wide.h -- the wide block of the matrix-free kernel operator: Out = (K(X, Y) + diag_add [X is Y]) V for 33 .. 128 right-hand
// sides in ONE launch (k_kmv_wide).  Float64, D <= 64, all four kernel kinds, symmetric and general.  Host side: agp_kmv_host.h
// (kmv_apply sends r > 32 here); r <= 32 stays on k_kmv (agp_kmv.h), whose slice sum k_kmv_sum serves both.
//
// Why: per 64 x 64 tile k_kmv pays for the kernel values once -- DP / 4 k-steps of the distance product per 16 columns, the kernel
// function, the close-point repair -- and spends them on 32 columns of V.  Here the same values, still in the accumulator registers
// of the first product, feed the second product for up to 128 columns: 16 k-steps x RB column blocks per 16 tile columns.
//
// THE BODY IS k_kmv's, not a copy of it: both kernels call kmv_body<KIND, DP, RB> (agp_kmv.h), which was written with RB as a
// parameter and the column-block loop innermost.  So the ownership (4 waves, 16 rows each, X fragments resident in registers), the
// transposed first product, the function step with the KMM_CLOSE repair, the hand-over of the finished tile in registers, the
// column-group split, and the order of the second product's k-steps are the same code, and column c of Out is the same chain of
// fused multiply-adds: for equal column groups the wide result equals the 32-column result bit for bit.  What this header adds is
// the instantiation at RB = 3, 4, 6, 8 and what had to be decided for it:
//   accumulators  16 x R per wave (R = 16 RB): RB d4 per lane, 32 doubles at RB = 8, live across all column tiles; one A operand (a
//                 finished kernel value) meets RB independent MFMA chains back to back.
//   V tile        64 x R in LDS as [j][c] with the row stride KMV_LDV<RB> (agp_kmv.h, generalised for this): R rounded up to 16
//                 (mod 32) = 48, 80, 112, 144.  Rows j and j + 1 then start half the banks apart, so the 32 lanes that one pass of a
//                 ds_read_b64 serves (two rows of 16 consecutive doubles) cover all 64 banks once: one full-rate read per B operand,
//                 as 48 does at R = 32.
//   prefetch      the next tile's V rows pass through registers as at R = 32: 4 RB doubles per lane (32 at RB = 8), loaded before
//                 the current tile's products and stored behind them.  With the accumulators (8 RB registers), the X fragments
//                 (DP / 2) and the Y prefetch (DP / 2) that is 16 RB + DP registers before the function step's temporaries and
//                 addresses: the compiler takes 256 plus up to 142 accumulation registers at RB = 6 and 8.  That is why the
//                 choice could be made at all: LDS limits the wide instances to one or two workgroups per CU anyway (below), so
//                 the launch bounds leave them 512 or 256 registers per lane, and every instance is scratch-free
//                 (profiles/r06_kernel_resources.txt).  A two-half prefetch would save 2 RB registers and add a barrier pair per
//                 tile; direct global-to-LDS loads cannot apply the row and column masks (gj < p, c < r) that let V have any
//                 leading dimension and any r.
//   LDS           2 x 64 (DP + 2) operand tiles + 64 LDV for V + 128 norms + DP scales, in KB (workgroups per CU that 160 KB allow):
//                            R = 48       R = 64       R = 96        R = 128
//                   DP = 16  44.2 (3)     60.5 (2)     76.9 (2)      93.3 (1)
//                   DP = 32  60.7 (2)     77.1 (2)     93.4 (1)     109.8 (1)
//                   DP = 64  93.7 (1)    110.1 (1)    126.5 (1)     142.8 (1)
//   launch bounds two workgroups per CU where LDS allows it and R <= 64, else one: a third workgroup would leave 170 registers per
//                 lane, and DP = 16, R = 96 at two (256 registers) spilled 100 to 236 bytes per lane.  (k_kmv's own bounds, by DP
//                 alone, stay as they are.)
#pragma once
#include "agp_kmv.h"

namespace agp {

constexpr int KMV_WIDE_MAXR = 128;  // right-hand sides per launch of k_kmv_wide
template <int DP, int RB>
constexpr int KMV_WIDE_WGS = (RB <= 4 && 2 * kmv_smem_bytes<DP, RB>() <= 160 * 1024) ? 2 : 1;  // workgroups per CU asked for

// The arguments of k_kmv; 32 < r <= 16 RB.  Dynamic LDS: kmv_smem_bytes<DP, RB>().
template <int KIND, int DP, int RB>
__global__ __launch_bounds__(NTHREADS, (KMV_WIDE_WGS<DP, RB>)) void k_kmv_wide(
    const double* __restrict__ X, int64_t ldx, int64_t n, const double* __restrict__ Ysc, const double* __restrict__ yng, int64_t p,
    int64_t D, const double* __restrict__ scales, double variance, int sym, double diag_add, const double* __restrict__ V, int64_t ldv,
    int r, double* __restrict__ out, int64_t ldo, int64_t slice) {
  static_assert(RB == 3 || RB == 4 || RB == 6 || RB == 8, "the wide instances: 48, 64, 96 and 128 columns");
  kmv_body<KIND, DP, RB>(X, ldx, n, Ysc, yng, p, D, scales, variance, sym, diag_add, V, ldv, r, out, ldo, slice);
}

}  // namespace agp
