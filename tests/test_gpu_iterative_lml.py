"""`IterativeGP.log_marginal_likelihood` / `optimize` (csrc/agp_kmv_grad.h, cg_solve_slq) against dense np.longdouble values.

Data recipe of tests/test_gpu_gp_cg.py, restated: unit cube, D = 3, scale 2, variance 1, noise 1e-2, cond < 1e5 asserted from the
reference matrix.  With base_samples = sqrt(t) I, t = n + rank_used, the probes satisfy sum_c z_c z_c' = t P, so the estimators of
log det(K + noise I) and tr((K + noise I)^-1 dK) are the exact quantities once CG has converged at tol = 1e-12.  Bounds:
  solve-dependent terms   4 cond tol |x_ref| per solved vector x (the form of test_gpu_gp_cg.py), carried through each product;
  the quadrature term     16 times the worst deviation of tests/_slq_ref.py (the same recurrence in NumPy Float64, on the CPU) from
                          the eigvalsh log-determinant over the shapes tested here -- measured against a reference, not the device;
  the bilinear forms      the budget of tests/_kmv_grad_ref.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _kmat_ref as KR
import _kmv_grad_ref as GR
import _slq_ref as SR

pytestmark = pytest.mark.gpu
LD = np.longdouble
NOISE, TOL, SCALE, D = 1e-2, 1e-12, 2.0, 3
SHAPES = [(65, 0), (65, 8), (130, 0), (130, 8)]


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _chol(M):
    n = len(M)
    L = np.zeros_like(M)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _inverse(L):
    n = len(L)
    Y = np.eye(n, dtype=LD)
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


def _data(n):
    rng = np.random.default_rng([n, 3])
    X = rng.random((n, D))
    return X, np.sin(3 * X[:, 0]) + np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _dense(n, scale=SCALE, noise=NOISE):
    """long double: log p, its gradients with respect to (variance, scales[D], noise), and what the bounds need"""
    X, y = _data(n)
    sx = KR.scaled(X, scale, "f64")
    d2, _ = KR.distances(sx, sx)
    K = KR.kernel_fn(0, d2)[0]
    M = K + LD(noise) * np.eye(n, dtype=LD)
    ev = np.linalg.eigvalsh(M.astype(np.float64))
    L = _chol(M)
    Minv = _inverse(L)
    alpha = Minv @ y.astype(LD)
    logp = -0.5 * (y.astype(LD) @ alpha) - np.sum(np.log(np.diag(L))) - 0.5 * n * np.log(2 * LD(np.pi))
    W = np.outer(alpha, alpha) - Minv  # d log p / d theta = 1/2 sum_ij W_ij dK_ij / d theta
    dK = [K] + [KR.kernel_fn(0, d2)[0] * -0.5 * (2 / LD(scale)) * (sx[:, None, d].astype(LD) - sx[None, :, d]) ** 2 for d in range(D)]
    grads = np.array([0.5 * np.sum(W * g) for g in dK] + [0.5 * np.trace(W)], dtype=LD)
    return dict(X=X, y=y, K=K, Minv=Minv, alpha=alpha, logp=logp, grads=grads, cond=float(ev[-1] / ev[0]))


@functools.lru_cache(maxsize=None)
def _slq_deviation():
    """worst |estimate - eigvalsh| of the NumPy restatement over SHAPES, and its factor L per shape"""
    dev, Ls = 0.0, {}
    for n, rank in SHAPES:
        est, ref, Ls[(n, rank)] = SR.exact_trace_logdet(_dense(n)["K"].astype(np.float64), NOISE, rank, TOL)
        dev = max(dev, abs(est - ref))
    return dev, Ls


def _model(AGP, n, rank, scale=SCALE):
    X, y = _data(n)
    m = AGP.IterativeGP(X, y, AGP.SqExponentialKernel() @ AGP.ScaleTransform(scale), noise=NOISE, tol=TOL, precond_rank=rank)
    m._solver()
    t = n + m.rank_used
    return m, np.sqrt(t) * np.eye(t)


@pytest.mark.parametrize("n,rank", SHAPES)
def test_exact_trace_identity(AGP, n, rank):
    ref = _dense(n)
    assert ref["cond"] < 1e5
    dev, Ls = _slq_deviation()
    m, base = _model(AGP, n, rank)
    logp, g = m.log_marginal_likelihood(base_samples=base, grad=True)
    assert m.info["converged"].all()
    m.close()
    t, ct = len(base), 4 * ref["cond"] * TOL
    nrm = lambda a: np.sqrt(np.sum(a * a, axis=0))  # noqa: E731
    # reference probes, solves and the pairs the bilinear kernel sees: (alpha, alpha; 1/2), (M^-1 z_c, P^-1 z_c; -1/(2t))
    Lf = Ls[(n, rank)].astype(LD)
    Z = np.sqrt(LD(t)) * np.column_stack([np.sqrt(LD(NOISE)) * np.eye(n, dtype=LD), Lf])
    Pinv = _inverse(_chol(Lf @ Lf.T + LD(NOISE) * np.eye(n, dtype=LD)))
    Uv, Vv = np.column_stack([ref["alpha"], ref["Minv"] @ Z]), np.column_stack([ref["alpha"], Pinv @ Z])
    w = np.concatenate([[0.5], np.full(t, -0.5 / t)])
    rv, rs, bv, bs = GR.reference(0, np.full(D, SCALE), 1.0, ref["X"], Uv.astype(np.float64), Vv.astype(np.float64), w)
    # a solved column u within ct |u|: u' (dK v) moves by at most ct |u| |dK v|; dK / d variance = K, |dK / d s_d| <= (2 / s) |K'| t^2 <= ...
    sx = KR.scaled(ref["X"], SCALE, "f64").astype(LD)
    dKs = [ref["K"]] + [ref["K"] * (sx[:, None, d] - sx[None, :, d]) ** 2 / LD(SCALE) for d in range(D)]
    solve = np.array([ct * np.sum(np.abs(w) * nrm(Uv) * nrm(g_ @ Vv) * (1 + (np.arange(t + 1) == 0))) for g_ in dKs])
    bound_logp = 0.5 * ct * nrm(ref["y"].astype(LD)) * nrm(ref["alpha"]) + 0.5 * 16 * dev + 8 * KR.U["f64"] * abs(ref["logp"])
    got = np.array([g["variance"]] + list(g["scales"]) + [g["noise"]], dtype=LD)
    bound_g = np.concatenate([solve + np.concatenate([[bv], bs]),
                              [ct * np.sum(np.abs(w) * nrm(Uv) * nrm(Vv) * (1 + (np.arange(t + 1) == 0)))
                               + KR.gamma(n + 8, KR.U["f64"]) * np.sum(np.abs(w) * nrm(Uv) * nrm(Vv))]])
    print(f"slq deviation {dev:.2e}; log p error / bound {float(abs(logp - ref['logp']) / bound_logp):.2e}; "
          f"gradient errors / bounds {np.array2string((np.abs(got - ref['grads']) / bound_g).astype(float), precision=2)}")
    assert abs(logp - ref["logp"]) <= bound_logp
    assert np.all(np.abs(got - ref["grads"]) <= bound_g)
    assert abs(g["scale"] - float(np.sum(g["scales"]))) <= 1e-15 * np.sum(np.abs(g["scales"]))


@pytest.mark.parametrize("rank", [0, 8])
def test_default_path_is_reproducible_and_the_table_changes_no_bit(AGP, rank):
    import torch
    from agp_amd import capi

    n, r = 130, 17
    m, _ = _model(AGP, n, rank)
    a = m.log_marginal_likelihood(num_probes=5, seed=3, grad=True)
    b = m.log_marginal_likelihood(num_probes=5, seed=3, grad=True)
    assert a[0] == b[0] and all(np.array_equal(np.asarray(a[1][k]), np.asarray(b[1][k])) for k in a[1])
    assert AGP.ELBO(m, num_probes=5, seed=3) == a[0] and m.log_marginal_likelihood(num_probes=5, seed=4) != a[0]
    B = torch.as_tensor(np.random.default_rng(0).standard_normal((n, r)), device="cuda")
    A = m.solve(B)
    info = m.info
    A2, Z0 = torch.empty_like(B), torch.empty_like(B)
    it, rr, cv, pb, qd = (C.c_int32 * r)(), (C.c_double * r)(), (C.c_int32 * r)(), (C.c_double * r)(), (C.c_double * r)()
    m._cx.chk(capi.lib().agp_gp_cg_solve_slq(m._h, C.c_void_p(B.data_ptr()), r, r, TOL, m.max_iter, m.check_every,
                                             C.c_void_p(A2.data_ptr()), r, C.c_void_p(Z0.data_ptr()), r, it, rr, cv, pb, qd))
    assert torch.equal(A.view(torch.int64), A2.view(torch.int64))
    assert list(it) == list(info["iterations"]) and list(rr) == list(info["residuals"])
    m.close()


def test_optimize_raises_the_dense_log_marginal_likelihood(AGP):
    n = 130
    start = _dense(n, scale=2 * SCALE)  # the lengthscale off by a factor of 2
    assert abs(float(np.sum(start["grads"][1:1 + D])) * 2 * SCALE) > 1.0  # d log p / d log scale at the start is not near zero
    m, base = _model(AGP, n, 8, scale=2 * SCALE)
    trace = m.optimize(5, optimiser=AGP.ADAM(0.05), base_samples=base)
    assert m.rank_used is None or m.rank_used == 8
    end = _dense(n, scale=float(m.kernel.transform.s), noise=float(m.noise))
    print(f"dense log p {float(start['logp']):.4f} -> {float(end['logp']):.4f}; scale {2 * SCALE} -> {m.kernel.transform.s:.4f}; "
          f"reported {trace[0]:.4f}")
    assert len(trace) == 5 and end["logp"] > start["logp"]
    m.close()
