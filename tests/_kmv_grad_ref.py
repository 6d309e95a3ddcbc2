"""Extended-precision reference and error budget of the derivative bilinear form `agp_kernel_bilinear_grad` (csrc/agp_kmv_grad.h), in the
manner of tests/_kmat_ref.py (whose scaled / distances / kernel_fn it builds on).  NumPy only.

Reference.  G = sum_c w_c u_c v_c', d2 by direct differences of the rounded scaled rows, all in np.longdouble:
    dvar = sum_ij G_ij phi(d2_ij) ,   dscale_d = (2 / s_d) sum_ij c_ij t_ijd^2 ,  c = G variance phi'(d2) ,  t_ijd = sx_id - sx_jd .

Budget (derived, not measured).  u = 2^-53, DP = D padded to 16 / 32 / 64, R = r padded to 16 per block of 32 pairs,
rho = 2 gamma_{DP+3} / KMM_CLOSE the relative error of d2 (tests/_kmat_ref.py, with this kernel's padding), C0 = 97 its function-evaluation
constant, k = n + 64 + partials + 16 the length of the longest chain of additions behind one output (column walk, 64 rows, partials).
    dG_ij    = gamma_{R+4} sum_c |w_c u_ic v_jc|                               (the G product, its blocks added)
    dphi_ij  = |phi'| d2 rho + (C0 + |a|) u |phi|      dphi'_ij = |phi''| d2 rho + (C0 + |a|) u |phi'|      (a: the exp argument)
    dc_ij    = variance (dG |phi'| + |G| dphi') + 3 u |c|
    |dvar - ref|     <= sum_ij (dG phi + |G| dphi) + gamma_k sum_ij |G phi|
    |dscale_d - ref| <= (2 / s_d) ( sum_ij dc_ij t_ijd^2 + gamma_k sum_{i != j} |c_ij| (|sx_id| + |sx_jd|)^2 ) + 4 u |ref|
The last sum is the expanded form sx^2 rho + Q - 2 sx O: each of its three products rounds relative to its own magnitude, not to t^2.
"""
import numpy as np

import _kmat_ref as KR

LD = np.longdouble
U64 = KR.U["f64"]


def dphi(kind, d2):
    """(phi', |phi''| d2) in long double"""
    d2 = np.asarray(d2, dtype=LD)
    r = np.sqrt(d2)
    if kind == 0:
        e = np.exp(-d2 / 2)
        return -e / 2, e * d2 / 4
    if kind == 1:
        s5 = np.sqrt(LD(5))
        e = np.exp(-s5 * r)
        return -(LD(5) / 6) * (1 + s5 * r) * e, LD(25) / 12 * e * d2
    s3 = np.sqrt(LD(3))
    e = np.exp(-s3 * r)
    return -LD(3) / 2 * e, LD(3) / 4 * s3 * r * e


def reference(kind, scales, variance, X, Uv, Vv, w, nparts=16):
    """(dvar, dscales[D], bound_var, bound_scales[D]) in long double"""
    n, D = X.shape
    r = Uv.shape[1]
    sx = KR.scaled(X, scales, "f64")
    d2, _ = KR.distances(sx, sx)
    phi, a, sens = KR.kernel_fn(kind, d2)
    dp_, ddp = dphi(kind, d2)
    Uw = Uv.astype(LD) * np.asarray(w, dtype=LD)
    G, Gabs = Uw @ Vv.astype(LD).T, np.abs(Uw) @ np.abs(Vv.astype(LD)).T
    DP = 16 if D <= 16 else 32 if D <= 32 else 64
    rho = 2.0 * KR.gamma(DP + 3, U64) / KR.THR["f64"]
    dG = KR.gamma(16 * ((min(r, 32) + 15) // 16) + 4, U64) * Gabs
    rnd = (KR.C0["f64"] + np.abs(a)) * U64
    gk = KR.gamma(n + 64 + nparts + 16, U64)
    var = LD(variance)
    dvar = np.sum(G * phi)
    bvar = np.sum(dG * phi + np.abs(G) * (sens * rho + rnd * phi)) + gk * np.sum(np.abs(G * phi)) + KR.TINY["f64"]
    c = G * var * dp_
    dc = var * (dG * np.abs(dp_) + np.abs(G) * (ddp * rho + rnd * np.abs(dp_))) + 3 * U64 * np.abs(c)
    coff = np.abs(c) * (1 - np.eye(n, dtype=LD))
    sxl, s = sx.astype(LD), np.broadcast_to(np.asarray(scales, dtype=np.float64), (D,)).astype(LD)
    dsc, bsc = np.zeros(D, dtype=LD), np.zeros(D, dtype=LD)
    for d in range(D):
        t2 = (sxl[:, None, d] - sxl[None, :, d]) ** 2
        big = (np.abs(sxl[:, None, d]) + np.abs(sxl[None, :, d])) ** 2
        dsc[d] = 2 / s[d] * np.sum(c * t2)
        bsc[d] = 2 / s[d] * (np.sum(dc * t2) + gk * np.sum(coff * big)) + 4 * U64 * abs(dsc[d]) + KR.TINY["f64"]
    return dvar, dsc, bvar, bsc
