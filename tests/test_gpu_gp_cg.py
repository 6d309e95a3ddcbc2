"""Batched preconditioned CG on the matrix-free operator (`agp_gp_cg_*`, csrc/agp_kmv_host.h) and `IterativeGP` on it, against a dense
np.longdouble K + sigma2 I (direct differences, tests/_kmat_ref.py) factored and solved in long double.

Variance 1 and noise 1e-2 give cond(K + sigma2 I) <= 100 n + 1; the tests compute cond from the reference matrix and assert it is
below 1e5, so the reference alone decides the margin.  With tol = 1e-12 every converged column must satisfy
    |A - A_ref| <= 4 cond tol |A_ref|      and      |B - (K + sigma2 I) A| <= 4 tol |B|   (long double residual)
(the factor 4: the gap between the recursive residual CG tests and the true one).
"""
import functools

import numpy as np
import pytest

import _kmat_ref as KR

pytestmark = pytest.mark.gpu
LD = np.longdouble
NOISE, TOL, SCALE, D = 1e-2, 1e-12, 2.0, 3  # lengthscale 0.5 on the unit cube: the spectrum of K decays fast


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _kernel(AGP):
    return AGP.SqExponentialKernel() @ AGP.ScaleTransform(SCALE)


def _chol_solve(M, B):
    """M \\ B in long double (NumPy's LAPACK drivers stop at double)"""
    n = len(M)
    L = np.zeros_like(M)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.array(B, dtype=LD)
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


@functools.lru_cache(maxsize=None)
def _system(n, dup=False):
    """X, M = K + sigma2 I in long double, cond(M) -- computed once per size and shared"""
    X = np.random.default_rng([n, 3]).random((n, D))
    if dup:
        X[n // 2:] = X[:n - n // 2]  # every point twice: K is singular, sigma2 keeps the system positive definite
    sx = KR.scaled(X, SCALE, "f64")
    M = KR.reference(0, "f64", 1.0, KR.distances(sx, sx)[0]) + LD(NOISE) * np.eye(n, dtype=LD)
    ev = np.linalg.eigvalsh(M.astype(np.float64))
    cond = float(ev[-1] / ev[0])
    assert cond < 1e5
    for a in (X, M):
        a.setflags(write=False)
    return X, M, cond


def _rhs(n, r, seed=0):
    B = np.random.default_rng([n, r, seed]).standard_normal((n, r))
    if r > 1:
        B[:, 1] = 0.0
    return B


def _check(M, cond, B, A, info):
    ref = _chol_solve(M, B)
    nrm = lambda a: np.sqrt(np.sum(a * a, axis=0))  # noqa: E731
    err, res = nrm(A.astype(LD) - ref), nrm(B.astype(LD) - M @ A.astype(LD))
    print(f"iterations {info['iterations'].max()}, worst error / bound {float(np.max(err / (4 * cond * TOL * nrm(ref) + 1e-300))):.2e}, "
          f"worst residual / bound {float(np.max(res / (4 * TOL * nrm(B) + 1e-300))):.2e}")
    assert info["converged"].all()
    assert np.all(err <= 4 * cond * TOL * nrm(ref)) and np.all(res <= 4 * TOL * nrm(B.astype(LD)))


@pytest.mark.parametrize("n,r,rank", [(1, 1, 0), (1, 1, 8), (64, 17, 8), (64, 32, 64), (65, 32, 0), (65, 1, 65), (130, 17, 8),
                                      (130, 32, 130), (130, 1, 0)])
def test_solve_against_the_long_double_solution(AGP, n, r, rank):
    X, M, cond = _system(n)
    B = _rhs(n, r)
    m = AGP.IterativeGP(X, np.zeros(n), _kernel(AGP), noise=NOISE, tol=TOL, precond_rank=rank)
    A = m.solve(B)
    _check(M, cond, B, A, m.info)
    if r > 1:  # the zero column: zeros, converged, no iteration
        assert not A[:, 1].any() and m.info["iterations"][1] == 0 and m.info["residuals"][1] == 0.0
    if rank >= n:  # an exact preconditioner
        assert m.rank_used == n and m.info["iterations"].max() <= 3
    m.close()


def test_preconditioner_cuts_iterations_and_duplicates_are_fine(AGP):
    X, M, cond = _system(130)
    B = _rhs(130, 17)
    its = {}
    for rank in (0, 8):
        m = AGP.IterativeGP(X, np.zeros(130), _kernel(AGP), noise=NOISE, tol=TOL, precond_rank=rank)
        m.solve(B)
        its[rank] = m.info["iterations"].max()
        m.close()
    assert its[0] > its[8], its
    Xd, Md, condd = _system(130, dup=True)
    for rank in (0, 130):  # (the pivoted Cholesky stops at the 65 distinct points)
        m = AGP.IterativeGP(Xd, np.zeros(130), _kernel(AGP), noise=NOISE, tol=TOL, precond_rank=rank)
        _check(Md, condd, B, m.solve(B), m.info)
        assert m.rank_used <= 65 * (rank > 0)
        m.close()


@pytest.mark.parametrize("rank", [0, 8])
def test_columns_are_independent_and_max_iter_is_reported(AGP, rank):
    X, M, cond = _system(130)
    B, B2 = _rhs(130, 17), _rhs(130, 17, seed=1) * 100.0
    B2[:, 5] = B[:, 5]
    m = AGP.IterativeGP(X, np.zeros(130), _kernel(AGP), noise=NOISE, tol=TOL, precond_rank=rank)
    A = m.solve(B)
    it5 = m.info["iterations"][5]
    A3 = m.solve(B2, max_iter=int(it5) + 7)  # other neighbours and another max_iter
    assert m.info["iterations"][5] == it5 and m.info["converged"][5]
    assert np.array_equal(A3[:, 5].view(np.int64), A[:, 5].view(np.int64))
    assert np.array_equal(m.solve(B)[:, 5].view(np.int64), A[:, 5].view(np.int64))
    A4 = m.solve(B, max_iter=2)  # not an error: reported
    assert not m.info["converged"][0] and m.info["iterations"][0] == 2 and m.info["converged"][1] and np.isfinite(A4).all()
    m.close()


@pytest.mark.parametrize("nt", [1, 33])
def test_model_against_the_dense_posterior_and_GP(AGP, nt):
    # The existing GP holds K + jitt I (jitt = 1e-4 in Float64, include/agp_hip.h) under its noise and reports k** + jitt - ...: the
    # model it is compared with therefore takes the noise sigma2 + jitt, and so does the dense reference.
    n, jitt = 130, 1e-4
    X, M, _ = _system(n)
    M = M + LD(jitt) * np.eye(n, dtype=LD)
    ev = np.linalg.eigvalsh(M.astype(np.float64))
    cond = float(ev[-1] / ev[0])
    rng = np.random.default_rng(nt)
    y, Xt, mean0 = np.sin(3 * X[:, 0]) + 0.1 * rng.standard_normal(n), rng.random((nt, D)), 0.3
    m = AGP.IterativeGP(X, y, _kernel(AGP), noise=NOISE + jitt, mean=mean0, tol=TOL, precond_rank=8)
    mu, var = AGP.predict_f(m, Xt)
    assert np.array_equal(AGP.predict_f(m, Xt, cov=False), mu) and np.array_equal(AGP.predict_y(m, Xt)[1], var + m.noise)
    # dense posterior in long double; ks = K(X, Xt) with its element-wise budget b
    d2, s2 = KR.distances(KR.scaled(X, SCALE, "f64"), KR.scaled(Xt, SCALE, "f64"))
    ks, b = KR.reference(0, "f64", 1.0, d2), KR.budget(0, "f64", D, 1.0, d2, s2)
    alpha, S = _chol_solve(M, (y - mean0)[:, None])[:, 0], _chol_solve(M, ks)
    nrm, g = (lambda a: np.sqrt(np.sum(a * a, axis=0))), KR.gamma(n + 16, KR.U["f64"])
    # the solve bound through k*, plus the products' own roundings (kernel values within b, dots of length n)
    bmu = 4 * cond * TOL * nrm(ks) * nrm(alpha) + np.abs(alpha) @ b + g * (np.abs(alpha) @ np.abs(ks)) + 2 * KR.U["f64"] * abs(mean0)
    bvar = 4 * cond * TOL * nrm(ks) * nrm(S) + 2 * np.sum(b * np.abs(S), axis=0) + g * np.sum(np.abs(ks * S), axis=0) + 4 * KR.U["f64"]
    assert np.all(np.abs(mu.astype(LD) - (ks.T @ alpha + mean0)) <= bmu)
    assert np.all(np.abs(var.astype(LD) - (1 - np.sum(ks * S, axis=0))) <= bvar)
    gp = AGP.GP(X, y - mean0, _kernel(AGP), noise=NOISE, optimiser=False, opt_noise=False)  # (the same alpha, zero prior mean)
    gmu, gvar = AGP.predict_f(gp, Xt, cov=True)
    assert np.all(np.abs(mu - mean0 - gmu) <= bmu) and np.all(np.abs(var + jitt - gvar) <= bvar)
    m2 = AGP.IterativeGP.from_model(gp, X, y - mean0, noise=NOISE + jitt, tol=TOL, precond_rank=8)
    assert np.array_equal(AGP.predict_f(m2, Xt, cov=False) + mean0, mu)
    with pytest.raises(NotImplementedError, match="GP"):
        AGP.train_(m, X, y, 1)
    with pytest.raises(NotImplementedError, match="diag=False"):
        AGP.predict_f(m, Xt, diag=False)
    m.close()
    m2.close()
