"""Extended-precision reference and error budget of the derivative of the fused kernel product with respect to its row points,
`agp_kernel_matmul_dx` (csrc/agp_kmv_dx.h), in the manner of tests/_kmv_grad_ref.py.  NumPy only.

Reference.  d2 and t_ijd = sx_id - sy_jd by direct differences of the rounded scaled rows, c = variance phi'(d2), all in np.longdouble:
    shared   out[i][c][d] = 2 s_d sum_j c_ij V_jc t_ijd          paired   out[i][d] = 2 s_d sum_j c_ij V_ji t_ijd

Budget (derived, not measured).  u = 2^-53, DP = D padded to 16 / 32 / 64, rho = 2 gamma_{DP+3} / KMM_CLOSE the relative
error of d2 (tests/_kmat_ref.py with this kernel's padding), C0 = 97 its function-evaluation constant.  The device evaluates
    out = 2 s_d ((sx_id - m_d) rho_ic - O_icd),   rho_ic = sum_j a_ijc,   O_icd = sum_j a_ijc (sy_jd - m_d),   a_ijc = fl(c_ij V_jc)
with m the scaled first row of the 64-row tile that row i belongs to (the anchor).
  c.    dc_ij = variance (|phi''| d2 rho + (C0 + |a|) u |phi'|) + 3 u |c_ij|            (tests/_kmv_grad_ref.py with G = 1, dG = 0)
  a.    one more multiply: |a_ijc - c_ij V_jc| <= dc_ij |V_jc| + u |c_ij V_jc|.  With exact sums these enter through t alone:
        sum_j (dc_ij |V_jc| + u |c_ij V_jc|) |t_ijd|.
  sums. sx - m and sy - m round once each, relative to |sx - m| and |sy - m|; rho is a chain of 16 additions per column tile in a lane,
        two across the lanes of a row and one per further column group; O is a chain of 64 multiply-adds per column tile on the matrix
        instruction and one addition per further group; then one product, one subtraction and the scaling by 2 s_d.  Each term of
        either sum is therefore off by at most gamma_k relative to ITS OWN magnitude, k = 64 ceil(p / 64) + groups + 8:
        gamma_k sum_j (|c_ij| + dc_ij) |V_jc| (|sx_id - m_d| + |sy_jd - m_d|)  -- distances from the anchor, not |t|: the cancellation term.
  |out - ref| <= 2 s_d [ sum_j (dc_ij |V_jc| + u |c_ij V_jc|) |t_ijd| + gamma_k sum_j (|c_ij| + dc_ij) |V_jc| (|sx_id - m_d| + |sy_jd - m_d|) ]
                 + 4 u |ref| + tiny.
"""
import numpy as np

import _kmat_ref as KR
from _kmv_grad_ref import dphi

LD = np.longdouble
U64 = KR.U["f64"]


def reference(kind, scales, variance, X, Y, V, paired=False, groups=16):
    """(ref, bound) in long double: (n, r, D), or (n, D) in paired mode (V: p x n).  groups: the column groups of the launch (the
    library takes at most 16 by itself)."""
    n, D = X.shape
    p = Y.shape[0]
    V = np.asarray(V, dtype=np.float64).reshape(p, -1)
    sx, sy = KR.scaled(X, scales, "f64").astype(LD), KR.scaled(Y, scales, "f64").astype(LD)
    d2, _ = KR.distances(sx, sy)
    _, a, _ = KR.kernel_fn(kind, d2)
    dp_, ddp = dphi(kind, d2)
    var = LD(variance)
    DP = 16 if D <= 16 else 32 if D <= 32 else 64
    c = var * dp_
    dc = var * (ddp * 2.0 * KR.gamma(DP + 3, U64) / KR.THR["f64"] + (KR.C0["f64"] + np.abs(a)) * U64 * np.abs(dp_)) + 3 * U64 * np.abs(c)
    gk = KR.gamma(64 * ((p + 63) // 64) + groups + 8, U64)
    m = sx[(np.arange(n) // 64) * 64]  # the anchor of every row
    s = np.broadcast_to(np.asarray(scales, dtype=np.float64), (D,)).astype(LD)
    Va = np.abs(V.astype(LD))
    ref = np.zeros((n, D) if paired else (n, V.shape[1], D), dtype=LD)
    bnd = np.zeros_like(ref)
    for d in range(D):
        t = sx[:, None, d] - sy[None, :, d]
        big = np.abs(sx[:, d] - m[:, d])[:, None] + np.abs(sy[None, :, d] - m[:, None, d])
        e1, e2 = (dc + U64 * np.abs(c)) * np.abs(t), gk * (np.abs(c) + dc) * big
        if paired:
            ref[:, d] = 2 * s[d] * np.sum(c * t * V.T, axis=1)
            bnd[:, d] = 2 * s[d] * np.sum((e1 + e2) * Va.T, axis=1)
        else:
            ref[:, :, d] = 2 * s[d] * ((c * t) @ V.astype(LD))
            bnd[:, :, d] = 2 * s[d] * ((e1 + e2) @ Va)
    return ref, bnd + 4 * U64 * np.abs(ref) + KR.TINY["f64"]
