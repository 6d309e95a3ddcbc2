"""`sample_paths(IterativeGP)`: the fused path-evaluation kernel (csrc/agp_path.h) and the matrix-free draw on it, against np.longdouble.

Evaluation bound, per element of out[i][c] = mean + sum_j Phi_ij W_jc + sum_r K_ir V_rc, from reference quantities only (u = 2^-53,
gamma_k = k u / (1 - k u)):
  kernel values    |K_ir - K_ref| <= b_ir = _kmat_ref.budget (the GEMM form of d2 with the repair of close points, as agp_kernel_matmul);
  feature values   the argument omega_j . (s o x_i) + p_j is a sum of D products and the phase, accumulated by the MFMA over the padded
                   dimension (the padding adds exact zeros): error <= gamma_{D+3} (sum_d |omega_jd s_d x_id| + |p_j|), which cos passes
                   on with slope <= 1; the device cos is within 2 ulp and the product by amp rounds once: 4 u.  So
                   |Phi_ij - Phi_ref| <= amp (gamma_{D+3} (sum_d |omega_jd s_d x_id| + |p_j|) + 4 u);
  the sum          one dot product of length N + L, tile by tile on the MFMA with R <= 32 padded columns, and up to 16 slices added in
                   order: gamma_{N+L+R} sum |term|.
  bound = sum_r b_ir |V_rc| + sum_j amp (gamma_{D+3} (sum_d |omega_jd s_d x_id| + |p_j|) + 4 u) |W_jc| + gamma_{N+L+32} sum |term|
The reference takes the DEVICE'S V (read back), so no CG error enters; amp is the double the device holds, sqrt(2 variance / L).
"""
import math

import numpy as np
import pytest

import _kmat_ref as KR
import _pathwise_ref as PR
from test_gpu_gp_cg import NOISE, SCALE, TOL, _chol_solve, _system

pytestmark = pytest.mark.gpu
LD, U = np.longdouble, KR.U["f64"]
KERNELS = ("SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel")


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _features_ref(X, scales, variance, tab):
    """(Phi_ref [n, L] in long double, its element bound) at the rows of X from the tables of a draw"""
    L, D = tab["omega"].shape
    sx, om, amp = KR.scaled(X, scales, "f64").astype(LD), tab["omega"].astype(LD), LD(math.sqrt(2.0 * variance / L))
    mag = np.abs(sx) @ np.abs(om).T + np.abs(tab["phase"].astype(LD))[None, :]
    return amp * np.cos(sx @ om.T + tab["phase"].astype(LD)[None, :]), amp * (KR.gamma(D + 3, U) * mag + 4 * U)


def _feature_bound(phi, dphi, W):
    """the feature part of the bound for Phi W: element errors through |W|, plus the dot product"""
    W = np.abs(W.astype(LD))
    return dphi @ W + KR.gamma(phi.shape[1] + 32, U) * (np.abs(phi) @ W)


# kind, D, ard, N, L, S, n_t, col_groups, mean.  Column tiles: ceil(L / 64) feature tiles, then ceil(N / 64) training tiles; with
# L = N = 200 (4 + 4), 3 groups take tiles 0-2 | 3-5 | 6-7 (one group walks the seam) and 5 groups 0-1 | 2-3 | 4-5 | 6 | 7: splits
# inside the feature segment and inside the training segment.  0: the library's choice (as many groups as tiles at these n_t).
CASES = [(0, 1, False, 1, 1, 1, 1, 0, 0.0), (1, 3, True, 65, 64, 17, 65, 0, 0.3), (2, 33, True, 200, 200, 33, 129, 3, 0.0),
         (3, 64, False, 200, 200, 17, 129, 5, -0.2), (0, 64, True, 65, 200, 33, 65, 1, 0.0), (1, 33, False, 200, 1, 1, 129, 2, 0.0),
         (2, 3, False, 1, 200, 17, 1, 2, 0.0), (3, 1, False, 65, 65, 33, 65, 4, 0.0)]


@pytest.mark.parametrize("kind,D,ard,N,L,S,nt,groups,mean", CASES)
def test_evaluation_within_the_derived_bound(AGP, kind, D, ard, N, L, S, nt, groups, mean):
    import torch

    rng = np.random.default_rng([kind, D, N, L, S, nt])
    variance = 1.3
    scales = (np.geomspace(0.3, 3.0, D) if ard else np.full(D, 1.1)) / math.sqrt(D)
    X, Xt = 2.0 + rng.random((N, D)), 2.0 + rng.random((nt, D))
    for i in range(0, nt, 5):  # every fifth test point: a copy of a training point, or its neighbour at 1e-7
        Xt[i] = X[i % N] + (1e-7 if i % 2 else 0.0)
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    k = variance * getattr(AGP, KERNELS[kind])() @ (AGP.ARDTransform(scales) if ard else AGP.ScaleTransform(scales[0]))
    m = AGP.IterativeGP(X, y, k, noise=1e-2, mean=mean if mean else None, precond_rank=8)
    paths = AGP.sample_paths(m, S, n_features=L, seed=11, t=3)
    F = paths(Xt, col_groups=groups)
    assert F.shape == (S, nt)
    tab = paths.tables()
    phi, dphi = _features_ref(Xt, scales, variance, tab)
    d2, s2 = KR.distances(KR.scaled(Xt, scales, "f64"), KR.scaled(X, scales, "f64"))
    K, b = KR.reference(kind, "f64", variance, d2), KR.budget(kind, "f64", D, variance, d2, s2)
    W, V = tab["W"].astype(LD), tab["V"].astype(LD)
    ref = LD(mean) + phi @ W + K @ V
    bound = b @ np.abs(V) + dphi @ np.abs(W) + KR.gamma(N + L + 32, U) * (np.abs(phi) @ np.abs(W) + np.abs(K) @ np.abs(V))
    ratio = np.abs(F.T.astype(LD) - ref) / bound
    print(f"worst error / bound {float(ratio.max()):.3f}")
    assert np.all(ratio <= 1.0)
    # the same bits on a second call and with pitched operands
    assert np.array_equal(_bits(paths(Xt, col_groups=groups)), _bits(F))
    wide = torch.zeros(nt, D + 3, dtype=torch.float64, device="cuda")
    wide[:, :D] = torch.as_tensor(Xt)
    assert np.array_equal(_bits(paths(wide[:, :D], col_groups=groups).cpu().numpy()), _bits(F))
    paths.free()
    m.close()


@pytest.mark.parametrize("rank", [0, 8])
@pytest.mark.parametrize("S", [3, 40])
def test_draw_tables_bit_for_bit_and_V_against_the_long_double_solve(AGP, rank, S):
    n, L, seed, t, mean0 = 130, 70, 2 ** 40 + 5, 2, 0.3
    X, M, cond = _system(n)  # (asserts cond < 1e5)
    D = X.shape[1]
    y = np.sin(3 * X[:, 0]) + 0.1 * np.random.default_rng(n).standard_normal(n)
    m = AGP.IterativeGP(X, y, AGP.SqExponentialKernel() @ AGP.ScaleTransform(SCALE), noise=NOISE, mean=mean0, tol=TOL, precond_rank=rank)
    paths = AGP.sample_paths(m, S, n_features=L, seed=seed, t=t)
    tab = paths.tables()
    om, ph = PR.features("sqexponential", D, L, seed, t)
    for name, ref in (("omega", om), ("phase", ph), ("W", PR.table(PR.W, L, S, seed, t)), ("E", PR.table(PR.E, n, S, seed, t))):
        assert np.array_equal(_bits(tab[name]), _bits(ref)), name
    assert paths.info["converged"].all() and len(paths.info["converged"]) == S
    phi, dphi = _features_ref(X, SCALE, 1.0, tab)
    R = (y - mean0).astype(LD)[:, None] - phi @ tab["W"].astype(LD) - np.sqrt(LD(NOISE)) * tab["E"].astype(LD)
    Vref, V = _chol_solve(M, R), tab["V"].astype(LD)
    nrm = lambda a: np.sqrt(np.sum(a * a, axis=0))  # noqa: E731
    err, res = nrm(V - Vref), nrm(R - M @ V)
    rbound = 4 * TOL * nrm(R) + nrm(_feature_bound(phi, dphi, tab["W"]))
    print(f"iterations {paths.info['iterations'].max()}, worst error / bound {float(np.max(err / (4 * cond * TOL * nrm(Vref)))):.2e}, "
          f"worst residual / bound {float(np.max(res / rbound)):.2e}")
    assert np.all(err <= 4 * cond * TOL * nrm(Vref)) and np.all(res <= rbound)
    paths.free()
    m.close()


def test_interface(AGP):
    X, _, _ = _system(65)
    y = np.cos(2 * X[:, 1])
    m = AGP.IterativeGP(X, y, AGP.SqExponentialKernel() @ AGP.ScaleTransform(SCALE), noise=NOISE)
    for bad in (dict(n_features=0), dict(n_features=8, n_samples=0)):
        with pytest.raises(ValueError):
            AGP.sample_paths(m, bad.pop("n_samples", 2), **bad)
    assert m._h is None  # refused before the device was touched
    Xt = np.random.default_rng(1).random((7, X.shape[1]))
    paths = AGP.sample_paths(m, 5, n_features=96, seed=4, t=1)  # (a TypeError before this feature)
    F = paths(Xt)
    assert F.shape == (5, 7) and np.isfinite(F).all() and "IterativeGP" in repr(paths)
    again, other = AGP.sample_paths(m, 5, n_features=96, seed=4, t=1), AGP.sample_paths(m, 5, n_features=96, seed=4, t=2)
    assert np.array_equal(_bits(again(Xt)), _bits(F)) and not np.array_equal(other(Xt), F)
    assert np.array_equal(_bits(paths(Xt.T.copy(), obsdim=2)), _bits(F))
    m.close()  # the paths are a snapshot
    assert np.array_equal(_bits(paths(Xt)), _bits(F))
    for call in (paths.grad, paths.maximize):
        with pytest.raises(NotImplementedError, match="IterativeGP"):
            call(Xt)
    for p in (paths, again, other):
        p.free()
    with pytest.raises(RuntimeError):
        paths(Xt)
