"""Long-double reference and derived bound for the Float32 kernel operator (csrc/agp_kmv_f32.h), on top of tests/_kmat_ref.py.
Per output element, with b32_ij = _kmat_ref.budget(kind, "f32", ...) on the centred coordinates, F = KMV32_F = 2, R = r padded to 16:
    |Out_ic - ref_ic| <= sum_j ( b32_ij |V_jc| + [V in Float64] 2^-24 |K_ij V_jc| + gamma32_{64 F + R} |K_ij V_jc| )
                         + gamma64_{ceil(p / 64 F) + 16} sum_j |K_ij V_jc| + [Out in Float32] 2^-24 |ref_ic|
Where the constants come from, in the code as built:
  b32       Rows are ((x - mean) * scale) in Float64, rounded to Float32 once (k_kmv32_prep): one relative u = 2^-24 per coordinate.
            d2 is the GEMM form on the Float32 MFMA over DP <= 64 padded dimensions where it stays above KMM_CLOSE<float> = 3e-2 of
            s2 = |sx|^2 + |sy|^2, Float32 direct differences below: _kmat_ref's d2 model with u = 2^-24, thr = 3e-2.  The input rounding
            moves d2 by at most 2 u sqrt(2 s2 d2): 17 u d2 where the GEMM form stays (rho >= 733 u); below the threshold a first-order
            kernel value moves by u g sqrt(2 s2) against the (16 + |a|) u g of the function evaluation, s2 that of the CENTRED rows.
            Function: v_exp_f32, the rounded log2(e) and its product, sqrt, the Matern polynomial, float(variance): C0 = 16.
  2^-24     V is rounded to Float32 when it is staged (Float64 storage); Out is rounded to Float32 (Float32 storage).
  64 F + R  A window is 64 F = 128 products accumulated in Float32 MFMA accumulators: at most 64 F roundings of the sum and one of
            each product; R is the allowance of the stated bound on top, not needed by the code.
  p/64F+16  One Float64 addition per window (at most ceil(p / 64 F) in a chain), at most 15 for the slices of 16 column groups, one
            FMA for diag_add V.
"""
import numpy as np

import _kmat_ref as KR

LD = np.longdouble
F = 2  # KMV32_F, csrc/agp_kmv_f32.h


def operator(kind, scales, variance, X, Y=None, diag_add=0.0):
    """(K-hat in long double by direct differences from the inputs as given, b32 on the centred coordinates); Y=None: symmetric"""
    sc = np.asarray(scales, dtype=np.float64).astype(LD)
    Yg = X if Y is None else Y
    d2, _ = KR.distances(X.astype(LD) * sc, Yg.astype(LD) * sc)
    K = KR.reference(kind, "f32", variance, d2)
    if Y is None:
        K = K + LD(diag_add) * np.eye(len(X), dtype=LD)
    mean = np.mean(X.astype(LD), axis=0)
    d2c, s2c = KR.distances((X.astype(LD) - mean) * sc, (Yg.astype(LD) - mean) * sc)
    return K, KR.budget(kind, "f32", X.shape[1], variance, d2c, s2c)


def bound(K, b, V, ref, v_f64, out_f32):
    """the bound of the module docstring for Out = K V, V p x r"""
    p, r = V.shape
    aV, u32 = np.abs(V.astype(LD)), KR.U["f32"]
    KV = np.abs(K) @ aV
    g32 = KR.gamma(64 * F + (r + 15) // 16 * 16, u32) + (u32 if v_f64 else 0.0)
    g64 = KR.gamma(-(-p // (64 * F)) + 16, KR.U["f64"])
    return b @ aV + (g32 + g64) * KV + (u32 * np.abs(ref) if out_f32 else 0.0)
