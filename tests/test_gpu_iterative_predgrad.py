"""`predict_f_grad(IterativeGP)` against the dense posterior: d k* by direct differences in long double (tests/_kmv_dx_ref.py), alpha and
(K + sigma2 I)^-1 k* by a dense Float64 solve, in the setting of tests/test_gpu_gp_cg.py (variance 1, noise 1e-2, tol 1e-12, cond < 1e5
asserted from the reference matrix).  With e = 4 cond tol (the project's solve margin) + cond n u (the dense solve's own error):
    |dmu[i, d]  - ref| <= e |d_d k*_i| |alpha|          + the operator's budget (shared mode on alpha)
    |dvar[i, d] - ref| <= 2 (e |d_d k*_i| |K^-1 k*_i|   + the operator's budget (paired mode on K^-1 k*))
"""
import numpy as np
import pytest

import _kmat_ref as KR
import _kmv_dx_ref as DR

pytestmark = pytest.mark.gpu
LD = np.longdouble
N, D, NOISE, TOL, SCALE, MEAN0 = 130, 3, 1e-2, 1e-12, 2.0, 0.3


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("nt", [1, 33])
def test_against_the_dense_posterior(AGP, nt, kind):
    rng = np.random.default_rng([nt, kind])
    X, Xt = rng.random((N, D)), rng.random((nt, D))
    y = np.sin(3 * X[:, 0]) + 0.1 * rng.standard_normal(N)
    sx, st = KR.scaled(X, SCALE, "f64"), KR.scaled(Xt, SCALE, "f64")
    M = (KR.reference(kind, "f64", 1.0, KR.distances(sx, sx)[0]) + LD(NOISE) * np.eye(N, dtype=LD)).astype(np.float64)
    ev = np.linalg.eigvalsh(M)
    cond = float(ev[-1] / ev[0])
    assert cond < 1e5
    ks = KR.reference(kind, "f64", 1.0, KR.distances(sx, st)[0]).astype(np.float64)
    alpha, S = np.linalg.solve(M, y - MEAN0), np.linalg.solve(M, ks)
    e = 4 * cond * TOL + cond * N * KR.U["f64"]
    eye = np.eye(N)  # column j of the shared mode on I is d k(x*_i, x_j) / d x*_i: the norms |d_d k*_i| of the bounds
    dk = np.sqrt(np.sum(DR.reference(kind, SCALE, 1.0, Xt, X, eye)[0] ** 2, axis=1))
    rmu, bmu = DR.reference(kind, SCALE, 1.0, Xt, X, alpha[:, None])
    rvar, bvar = DR.reference(kind, SCALE, 1.0, Xt, X, S, paired=True)
    rmu, bmu = rmu[:, 0], bmu[:, 0] + e * dk * np.linalg.norm(alpha)
    rvar, bvar = -2 * rvar, 2 * (bvar + e * dk * np.linalg.norm(S, axis=0)[:, None])

    k = [AGP.SqExponentialKernel, AGP.Matern52Kernel, AGP.Matern32Kernel][kind]() @ AGP.ScaleTransform(SCALE)
    m = AGP.IterativeGP(X, y, k, noise=NOISE, mean=MEAN0, tol=TOL, precond_rank=8)
    dmu, dvar = AGP.predict_f_grad(m, Xt)
    assert dmu.shape == dvar.shape == (nt, D) and m.alpha_info["converged"].all() and m.info["converged"].all()
    print(f"dmu error / bound {float(np.max(np.abs(dmu - rmu) / bmu)):.2e}, dvar error / bound {float(np.max(np.abs(dvar - rvar) / bvar)):.2e}")
    assert np.all(np.abs(dmu - rmu) <= bmu) and np.all(np.abs(dvar - rvar) <= bvar)
    info = m.info
    only = AGP.predict_f_grad(m, Xt, cov=False)
    assert m.info is info and np.array_equal(only.view(np.int64), dmu.view(np.int64))  # no further solve
    g2 = AGP.predict_f_grad(m, np.ascontiguousarray(Xt.T), obsdim=2)
    assert np.array_equal(g2[0].view(np.int64), dmu.view(np.int64)) and np.array_equal(g2[1].view(np.int64), dvar.view(np.int64))
    m.close()
