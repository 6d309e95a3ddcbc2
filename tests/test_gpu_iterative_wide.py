"""`IterativeGP(block=128)`: 128 columns per batched CG run on the wide operator kernel (csrc/agp_kmv_wide.h, agp_gp_cg_set_block).
System, right-hand sides, long-double solve and bounds are those of tests/test_gpu_gp_cg.py (4 cond tol |x_ref| per solved column,
cond from the reference matrix); the block-32 model on the same data is the second witness.
"""
import numpy as np
import pytest

import _kmat_ref as KR
import test_gpu_gp_cg as G
from test_gpu_gp_cg import AGP  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _model(AGP, n, rank, block, y=None, **kw):  # noqa: F811
    X = G._system(n)[0]
    return AGP.IterativeGP(X, np.zeros(n) if y is None else y, G._kernel(AGP), noise=G.NOISE, tol=G.TOL, precond_rank=rank, block=block, **kw)


def _y(n):
    return np.sin(3 * G._system(n)[0][:, 0]) + 0.1 * np.random.default_rng(n).standard_normal(n)


# (n = 300: two workgroups of 256 rows per panel, three panels -- the per-panel offsets of the partial sums with nblk > 1)
@pytest.mark.parametrize("n,r,rank", [(65, 33, 0), (65, 128, 8), (130, 128, 0), (130, 130, 8), (130, 33, 130), (300, 65, 8)])
def test_solve_against_the_long_double_solution(AGP, n, r, rank):  # noqa: F811
    _, M, cond = G._system(n)
    B = G._rhs(n, r)
    m = _model(AGP, n, rank, 128)  # (a TypeError before the wide block)
    A = m.solve(B)
    assert len(m.info["converged"]) == r
    G._check(M, cond, B, A, m.info)  # every column converged, error and residual within the bounds
    assert not A[:, 1].any() and m.info["iterations"][1] == 0
    m32 = _model(AGP, n, rank, 32)  # one wide product against two narrow ones: the same bits
    assert np.array_equal(m.operator(A[:, :40]).view(np.int64), m32.operator(A[:, :40]).view(np.int64))
    m.close()
    m32.close()


@pytest.mark.parametrize("n", [65, 130])
def test_prediction_within_the_dense_bounds_and_the_mean_bitwise(AGP, n):  # noqa: F811
    X, M, cond = G._system(n)
    y, Xt, D = _y(n), np.random.default_rng(40).random((40, G.D)), G.D
    m, m32 = _model(AGP, n, 8, 128, y), _model(AGP, n, 8, 32, y)
    mu, var = AGP.predict_f(m, Xt)
    assert np.array_equal(mu.view(np.int64), AGP.predict_f(m32, Xt, cov=False).view(np.int64))
    d2, s2 = KR.distances(KR.scaled(X, G.SCALE, "f64"), KR.scaled(Xt, G.SCALE, "f64"))
    ks, b = KR.reference(0, "f64", 1.0, d2), KR.budget(0, "f64", D, 1.0, d2, s2)
    alpha, S = G._chol_solve(M, y[:, None])[:, 0], G._chol_solve(M, ks)
    nrm, g = (lambda a: np.sqrt(np.sum(a * a, axis=0))), KR.gamma(n + 16, KR.U["f64"])
    bmu = 4 * cond * G.TOL * nrm(ks) * nrm(alpha) + np.abs(alpha) @ b + g * (np.abs(alpha) @ np.abs(ks))
    bvar = 4 * cond * G.TOL * nrm(ks) * nrm(S) + 2 * np.sum(b * np.abs(S), axis=0) + g * np.sum(np.abs(ks * S), axis=0) + 4 * KR.U["f64"]
    assert np.all(np.abs(mu.astype(LD) - ks.T @ alpha) <= bmu)
    assert np.all(np.abs(var.astype(LD) - (1 - np.sum(ks * S, axis=0))) <= bvar)
    assert np.array_equal(AGP.predict_y(m, Xt)[1], var + m.noise)
    m.close()
    m32.close()


@pytest.mark.parametrize("n", [65, 130])
def test_log_marginal_likelihood_in_one_pass_agrees_with_two(AGP, n):  # noqa: F811
    """33 columns: one CG run at block 128, two at block 32.  Bound: each run's solve term of tests/test_gpu_iterative_lml.py,
    1/2 (4 cond tol) |y| |alpha|, added."""
    _, M, cond = G._system(n)
    y = _y(n)
    m, m32 = _model(AGP, n, 8, 128, y), _model(AGP, n, 8, 32, y)
    a, b = m.log_marginal_likelihood(num_probes=32, seed=0), m32.log_marginal_likelihood(num_probes=32, seed=0)
    assert len(m.info["converged"]) == 33 and m.info["converged"].all()
    alpha = G._chol_solve(M, y[:, None])[:, 0]
    bound = 2 * 0.5 * 4 * cond * G.TOL * float(np.sqrt(y @ y) * np.sqrt(alpha @ alpha))
    print(f"log p {a:.6f} against {b:.6f}; difference / bound {abs(a - b) / bound:.2e}")
    assert abs(a - b) <= bound
    m.close()
    m32.close()


@pytest.mark.parametrize("n", [65, 130])
def test_path_draws_are_finite_and_reproducible(AGP, n):  # noqa: F811
    Xt = np.random.default_rng(1).random((7, G.D))
    m = _model(AGP, n, 8, 128, _y(n))
    F = [AGP.sample_paths(m, 40, n_features=96, seed=4, t=1) for _ in range(2)]
    assert F[0].info["converged"].all() and len(F[0].info["converged"]) == 40
    out = [p(Xt) for p in F]
    assert out[0].shape == (40, 7) and np.isfinite(out[0]).all() and np.array_equal(out[0].view(np.int64), out[1].view(np.int64))
    for p in F:
        p.free()
    m.close()


def test_refusals(AGP):  # noqa: F811
    with pytest.raises(ValueError, match="block must be 32 or 128"):
        _model(AGP, 65, 0, 64)
    with pytest.raises(ValueError, match="Float32"):
        _model(AGP, 65, 0, 128, operator_dtype=np.float32)
