"""`IterativeGP` with 65 <= D <= 128: the batched CG, the predictions and the log marginal likelihood on the operator kernel for that
range (csrc/agp_kmv_hd.h).  The recipe, reference solve and bounds are those of tests/test_gpu_gp_cg.py (4 cond tol |x| per solved
column; `bmu`, `bvar`) and tests/test_gpu_iterative_lml.py (the exact-trace setting base_samples = sqrt(t) I), restated where those
files fix D = 3; the scale is theirs times sqrt(3 / D), so the kernel matrix is as far from the identity as it is there.
"""
import functools

import numpy as np
import pytest

import _kmat_ref as KR
import _slq_ref as SR
import test_gpu_gp_cg as G
from test_gpu_gp_cg import AGP  # noqa: F401  (the fixture)
from test_gpu_iterative_lml import _chol

pytestmark = pytest.mark.gpu
LD = np.longdouble
N, NT, JITT, MEAN0 = 130, 33, 1e-4, 0.3  # (JITT: what AGP.GP holds under its noise, as in test_gpu_gp_cg.py)
SHAPES = [(65, 0), (65, 8), (128, 0), (128, 8)]


def _kernel(AGP, D):  # noqa: F811
    return AGP.SqExponentialKernel() @ AGP.ScaleTransform(G.SCALE * np.sqrt(3.0 / D))


@functools.lru_cache(maxsize=None)
def _system(D):
    """data, K and M = K + (noise + jitt) I in long double with its condition number, test points: once per D, shared"""
    rng = np.random.default_rng([N, D])
    X, Xt = rng.random((N, D)), rng.random((NT, D))
    y = np.sin(3 * X[:, 0]) + 0.1 * rng.standard_normal(N)
    sx = KR.scaled(X, G.SCALE * np.sqrt(3.0 / D), "f64")
    K = KR.reference(0, "f64", 1.0, KR.distances(sx, sx)[0])
    M = K + LD(G.NOISE + JITT) * np.eye(N, dtype=LD)
    ev = np.linalg.eigvalsh(M.astype(np.float64))
    assert ev[-1] / ev[0] < 1e5
    return dict(X=X, Xt=Xt, y=y, sx=sx, K=K, M=M, cond=float(ev[-1] / ev[0]))


@pytest.mark.parametrize("D,rank", SHAPES)
def test_solve_predictions_and_log_marginal_likelihood(AGP, D, rank):  # noqa: F811
    s = _system(D)
    X, Xt, y, M, cond, noise = s["X"], s["Xt"], s["y"], s["M"], s["cond"], G.NOISE + JITT
    m = AGP.IterativeGP(X, y, _kernel(AGP, D), noise=noise, mean=MEAN0, tol=G.TOL, precond_rank=rank)
    B = G._rhs(N, 17)
    G._check(M, cond, B, m.solve(B), m.info)  # (AGPError from agp_gp_cg_create before D > 64 was served)
    # predict_f / predict_y against the dense posterior in long double, inside bmu and bvar of test_gpu_gp_cg.py, and against GP
    mu, var = AGP.predict_f(m, Xt)
    assert np.array_equal(AGP.predict_y(m, Xt)[1], var + m.noise)
    d2, s2 = KR.distances(s["sx"], KR.scaled(Xt, G.SCALE * np.sqrt(3.0 / D), "f64"))
    ks, b = KR.reference(0, "f64", 1.0, d2), KR.budget(0, "f64", D, 1.0, d2, s2)
    alpha, S = G._chol_solve(M, (y - MEAN0)[:, None])[:, 0], G._chol_solve(M, ks)
    nrm, g, ct = (lambda a: np.sqrt(np.sum(a * a, axis=0))), KR.gamma(N + 16, KR.U["f64"]), 4 * cond * G.TOL
    bmu = ct * nrm(ks) * nrm(alpha) + np.abs(alpha) @ b + g * (np.abs(alpha) @ np.abs(ks)) + 2 * KR.U["f64"] * abs(MEAN0)
    bvar = ct * nrm(ks) * nrm(S) + 2 * np.sum(b * np.abs(S), axis=0) + g * np.sum(np.abs(ks * S), axis=0) + 4 * KR.U["f64"]
    assert np.all(np.abs(mu.astype(LD) - (ks.T @ alpha + MEAN0)) <= bmu)
    assert np.all(np.abs(var.astype(LD) - (1 - np.sum(ks * S, axis=0))) <= bvar)
    gp = AGP.GP(X, y - MEAN0, _kernel(AGP, D), noise=G.NOISE, optimiser=False, opt_noise=False)
    gmu, gvar = AGP.predict_f(gp, Xt, cov=True)
    assert np.all(np.abs(mu - MEAN0 - gmu) <= bmu) and np.all(np.abs(var + JITT - gvar) <= bvar)
    # log p(y) with exact traces: the bound of test_gpu_iterative_lml.py, its quadrature term from the NumPy restatement at this shape
    t = N + m.rank_used
    logp = m.log_marginal_likelihood(base_samples=np.sqrt(t) * np.eye(t))
    assert m.info["converged"].all()
    assert AGP.ELBO(m, num_probes=5, seed=3) == m.log_marginal_likelihood(num_probes=5, seed=3)  # (random probes: reproducible)
    est, ref_logdet, _ = SR.exact_trace_logdet(s["K"].astype(np.float64), noise, rank, G.TOL)
    ref = -0.5 * ((y - MEAN0).astype(LD) @ alpha) - np.sum(np.log(np.diag(_chol(M)))) - 0.5 * N * np.log(2 * LD(np.pi))
    bound = 0.5 * ct * nrm((y - MEAN0).astype(LD)) * nrm(alpha) + 0.5 * 16 * abs(est - ref_logdet) + 8 * KR.U["f64"] * abs(ref)
    print(f"log p error / bound {float(abs(logp - ref) / bound):.2e}")
    assert abs(logp - ref) <= bound
    m.close()


def test_what_stops_at_64_dimensions_is_refused_by_name(AGP):  # noqa: F811
    s = _system(65)
    m = AGP.IterativeGP(s["X"], s["y"], _kernel(AGP, 65), noise=G.NOISE + JITT, tol=G.TOL, precond_rank=8)
    for call in (lambda: AGP.predict_f_grad(m, s["Xt"]), lambda: AGP.sample_paths(m, 4), lambda: m.optimize(1),
                 lambda: m.log_marginal_likelihood(grad=True)):
        with pytest.raises(NotImplementedError, match="D = 65.*64"):
            call()
    for kw in (dict(operator_dtype=np.float32), dict(block=128)):
        with pytest.raises(ValueError, match="D = 65.*64"):
            AGP.IterativeGP(s["X"], s["y"], _kernel(AGP, 65), **kw)
    B = G._rhs(N, 3)
    G._check(s["M"], s["cond"], B, m.solve(B), m.info)  # the model still solves
    m.close()
