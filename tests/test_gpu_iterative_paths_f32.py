"""`paths(X, dtype=np.float32)` on an IterativeGP's draw: the Float32 fused path-evaluation kernel (csrc/agp_path_f32.h) against
np.longdouble, by direct differences from the inputs as given, with the device's own Float64 tables (no CG error enters).

Bound per element of out[i][c] = mean + sum_j Phi_ij W_jc + sum_r K_ir V_rc, from reference quantities only (u = 2^-24, u64 = 2^-53,
gamma_k = k u / (1 - k u), mu = the training mean, F = 2 tiles per Float32 window):
  kernel values   |K_ir - K_ref| <= b32_ir = _kmat_ref.budget(kind, "f32", ...) on the coordinates centred by mu (tests/_kmv32_ref.py:
                  rows rounded to Float32 once after centring and scaling in Float64, the GEMM form of d2 above KMM_CLOSE<float> and
                  direct differences below, the Float32 function evaluation);
  feature values  the Float32 argument is omega_j . (s o (x_i - mu)) + p'_j with p'_j = p_j + omega_j . (s o mu) reduced to [-pi, pi) in
                  Float64 and rounded once (u |p'_j|).  omega and the centred row are rounded once each, the MFMA adds D products with
                  one rounding per step (the padding adds exact zeros) and the phase is added: gamma_{D+3} sum_d |omega_jd s_d (x_id -
                  mu_d)|.  cos has slope <= 1; cosf, the rounded amp and the product with it: 4 u.  So
                  |Phi_ij - Phi_ref| <= amp (gamma_{D+3} sum_d |omega_jd s_d (x_id - mu_d)| + u |p'_j| + 4 u);
  W and V         rounded to Float32 once: u |term|;
  a window        at most 64 F products summed in Float32 MFMA accumulators, 32 on top as in _kmv32_ref: gamma_{64 F + 32} |term|;
  Float64 chain   one addition per window and per slice of at most 16 column groups: gamma64_{ceil(tiles / F) + 16} sum |term|;
  the store       to Float32: u |ref|.
  bound = sum_r b32_ir |V_rc| + sum_j dPhi_ij |W_jc| + (u + gamma_{64 F + 32} + gamma64_{ceil(tiles / F) + 16}) sum |term| + u |ref|
Not in the bound: with a constant prior mean the wrapper adds it in Float64 and rounds a second time (u |ref - mean| more), and the
addition of the phase rounds relative to |argument + p'|, u |p'_j| more than the gamma_{D+3} term carries.  Both are worst cases of
single roundings next to a window term of 160 u sum |term|; the case with a mean is there to show it.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _kmat_ref as KR
import _kmv32_ref as K32

pytestmark = pytest.mark.gpu
LD, U32, U64 = np.longdouble, KR.U["f32"], KR.U["f64"]
KERNELS = ("SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel")


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# kind, D, ard, N, L, S, n_t, col_groups, mean.  Tiles: ceil(L / 64) feature tiles, then ceil(N / 64) training tiles; a Float32 window is
# two tiles and starts with the column group.  L = 64, N = 200, one group: the first window holds the feature tile and a training tile.
# L = 128: the seam is a window boundary.  L = N = 200 (4 + 4 tiles): 3 groups take 0-2 | 3-5 | 6-7 and 5 groups 0-1 | 2-3 | 4-5 | 6 | 7,
# so groups start inside what would be a window of the whole list and the second of 3 walks the seam inside its first window.  S = 33:
# two launches, the second with 16 columns or fewer.  col_groups = 0: the library's choice.
CASES = [(0, 1, False, 1, 1, 1, 1, 0, 0.0), (1, 3, True, 200, 64, 17, 65, 1, 0.3), (2, 33, True, 200, 128, 33, 129, 1, 0.0),
         (3, 64, False, 200, 200, 17, 129, 3, 0.0), (0, 64, True, 200, 200, 33, 65, 5, 0.0), (1, 33, False, 200, 1, 1, 129, 2, 0.0),
         (2, 3, False, 1, 200, 17, 1, 2, 0.0), (3, 1, False, 65, 65, 33, 65, 0, 0.0), (0, 33, False, 65, 128, 17, 65, 0, 0.0)]


@pytest.mark.parametrize("kind,D,ard,N,L,S,nt,groups,mean", CASES)
def test_float32_evaluation_within_the_derived_bound_and_its_bits(AGP, kind, D, ard, N, L, S, nt, groups, mean):
    import torch

    rng = np.random.default_rng([kind, D, N, L, S, nt])
    variance = 1.3
    scales = (np.geomspace(0.3, 3.0, D) if ard else np.full(D, 1.1)) / math.sqrt(D)
    X, Xt = 10.0 + rng.random((N, D)), 10.0 + rng.random((nt, D))
    for i in range(0, nt, 5):  # every fifth test point: a copy of a training point, or its neighbour at 1e-4
        Xt[i] = X[i % N] + (1e-4 if i % 2 else 0.0)
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    k = variance * getattr(AGP, KERNELS[kind])() @ (AGP.ARDTransform(scales) if ard else AGP.ScaleTransform(scales[0]))
    m = AGP.IterativeGP(X, y, k, noise=1e-2, mean=mean if mean else None, precond_rank=8)
    paths = AGP.sample_paths(m, S, n_features=L, seed=11, t=3)
    F64 = paths(Xt, col_groups=groups)
    F = paths(Xt, col_groups=groups, dtype=np.float32)
    assert F.shape == (S, nt) and F.dtype == np.float32
    tab = paths.tables()
    sc, mu = scales.astype(LD), X.astype(LD).mean(axis=0)
    om, ph, W, V = (tab[q].astype(LD) for q in ("omega", "phase", "W", "V"))
    amp = LD(math.sqrt(2.0 * variance / L))
    phi = amp * np.cos((Xt.astype(LD) * sc) @ om.T + ph[None, :])
    php = ph + om @ (sc * mu)
    php = php - 2 * LD(np.pi) * np.rint(php / (2 * LD(np.pi)))  # (np.pi against the long-double pi: 1e-16, nothing at u = 6e-8)
    dphi = amp * (KR.gamma(D + 3, U32) * (np.abs((Xt.astype(LD) - mu) * sc) @ np.abs(om).T) + U32 * np.abs(php)[None, :] + 4 * U32)
    d2, _ = KR.distances(Xt.astype(LD) * sc, X.astype(LD) * sc)
    d2c, s2c = KR.distances((Xt.astype(LD) - mu) * sc, (X.astype(LD) - mu) * sc)
    K, b = KR.reference(kind, "f32", variance, d2), KR.budget(kind, "f32", D, variance, d2c, s2c)
    ref = LD(mean) + phi @ W + K @ V
    tiles = -(-L // 64) + -(-N // 64)
    chain = U32 + KR.gamma(64 * K32.F + 32, U32) + KR.gamma(-(-tiles // K32.F) + 16, U64)
    bound = b @ np.abs(V) + dphi @ np.abs(W) + chain * (np.abs(phi) @ np.abs(W) + np.abs(K) @ np.abs(V)) + U32 * np.abs(ref)
    ratio = np.abs(F.T.astype(LD) - ref) / bound
    print(f"worst error / bound {float(ratio.max()):.2e}")
    assert np.all(ratio <= 1.0)
    # bits: a second call, pitched operands, obsdim=2, the Float64 evaluation after the first Float32 call, the snapshot
    assert np.array_equal(_bits(paths(Xt, col_groups=groups, dtype=np.float32)), _bits(F))
    wide = torch.zeros(nt, D + 3, dtype=torch.float64, device="cuda")
    wide[:, :D] = torch.as_tensor(Xt)
    assert np.array_equal(_bits(paths(wide[:, :D], col_groups=groups, dtype=np.float32).cpu().numpy()), _bits(F))
    assert np.array_equal(_bits(paths(Xt.T.copy(), obsdim=2, col_groups=groups, dtype=np.float32)), _bits(F))
    assert np.array_equal(_bits(paths(Xt, col_groups=groups)), _bits(F64))
    m.close()
    assert np.array_equal(_bits(paths(Xt, col_groups=groups, dtype=np.float32)), _bits(F))
    paths.free()


def test_interface(AGP):
    import torch
    from agp_amd import capi

    rng = np.random.default_rng(5)
    X, Xt = rng.random((65, 3)), rng.random((7, 3))
    m = AGP.IterativeGP(X, np.cos(2 * X[:, 1]), AGP.SqExponentialKernel() @ AGP.ScaleTransform(1.5), noise=1e-2)
    paths = AGP.sample_paths(m, 5, n_features=96, seed=4, t=1)
    F = paths(Xt, dtype=np.float32)  # (a TypeError before this feature)
    assert F.dtype == np.float32 and F.shape == (5, 7) and np.isfinite(F).all()
    assert paths(torch.as_tensor(Xt, device="cuda"), dtype=np.float32).dtype == torch.float32
    assert paths(Xt[:0], dtype=np.float32).shape == (5, 0)
    with pytest.raises(ValueError, match="np.float64 or np.float32"):
        paths(Xt, dtype=np.float16)
    for call in (paths.grad, paths.maximize):
        with pytest.raises(NotImplementedError, match="IterativeGP"):
            call(Xt)
    # the raw entry point: an empty evaluation and a null out are refused by name, before anything is touched
    L = capi.lib()
    xd = torch.as_tensor(Xt, device="cuda")
    out = torch.full((7, 5), float("nan"), dtype=torch.float32, device="cuda")
    px, po = C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr())
    for word, args in (("n_t >= 1", (px, 3, 0, 0, po, 5)), ("xt and out must be given", (px, 3, 7, 0, None, 5)),
                       ("ldo >= n_samples", (px, 3, 7, 0, po, 4)), ("ldx >= D", (px, 2, 7, 0, po, 5))):
        st = L.agp_gp_cg_pathwise_eval_f32(paths._p, *args)
        msg = L.agp_last_error(paths._cx.ctx).decode()
        assert st == 1 and "agp_gp_cg_pathwise_eval_f32" in msg and word in msg, (word, st, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    paths.free()
    m.close()
