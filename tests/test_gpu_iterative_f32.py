"""`IterativeGP(operator_dtype=np.float32)`: the batched CG and the log marginal likelihood on the Float32 operator
(csrc/agp_kmv_f32.h).  Data recipe of tests/test_gpu_iterative_lml.py: unit cube, D = 3, scale 2, variance 1, noise 1e-2, n = 130.
The solve.  The recursive residual reaches tol; each iteration can add at most one operator error to its distance from the true one,
so with E the bound of tests/_kmv32_ref.py applied to |x|:  |b - K-hat x| / |b| <= tol + (iterations + 1) |E(|x|)| / |b|.
The likelihood.  First order in the element budget dK = b32, with M = K + noise I, alpha = M^-1 y, G = dM / d theta (Float64 in both runs):
  value      1/2 sum |alpha_i| dK_ij |alpha_j| + 1/2 sum |M^-1_ij| dK_ij       (d log p = 1/2 alpha' dK alpha - 1/2 tr(M^-1 dK))
  gradient   1/2 alpha' G alpha - 1/2 tr(M^-1 G) sees the Float32 operator through d alpha = -M^-1 dK alpha and d M^-1 = -M^-1 dK M^-1:
             the same expression with G carried through the solves, sum |(M^-1 G alpha)_i| dK_ij |alpha_j| + 1/2 sum |(M^-1 G M^-1)_ij| dK_ij.
Each run adds what a solve at tol = 1e-10 leaves (every solved x within ct |x|, ct = 4 cond tol as in test_gpu_iterative_lml.py):
the value 1/2 ct |y| |alpha| and that file's quadrature allowance; a gradient entry ct |alpha| |G alpha| and, for the exact-trace probes
(Z Z' = t P, sigma2 I <= P <= M), 1/2 ct |M^-1 Z|_F |G P^-1 Z|_F / t <= 1/2 ct sqrt(tr(M^-1) / sigma2) |G|_F.
"""
import functools

import numpy as np
import pytest

import _kmat_ref as KR
import _kmv32_ref as R32
import _kmv_grad_ref as GR
from test_gpu_iterative_lml import AGP, D, NOISE, SCALE, _data, _slq_deviation  # noqa: F401

pytestmark = pytest.mark.gpu
N = 130
KERNELS = {0: "SqExponentialKernel", 1: "Matern52Kernel", 2: "Matern32Kernel"}


@functools.lru_cache(maxsize=None)
def _dense(kind):
    """K + noise I in long double from X as given, b32, M^-1 (a Float64 inverse: only magnitudes are taken from it), cond"""
    X, y = _data(N)
    K, b = R32.operator(kind, np.full(D, SCALE), 1.0, X, None, NOISE)
    Minv = np.linalg.inv(K.astype(np.float64))
    return X, y, K, b, Minv, np.linalg.cond(K.astype(np.float64))


def _model(AGP, kind, rank, tol, dtype):
    return AGP.IterativeGP(*_data(N), getattr(AGP, KERNELS[kind])() @ AGP.ScaleTransform(SCALE), noise=NOISE, tol=tol, precond_rank=rank,
                           operator_dtype=dtype)


@pytest.mark.parametrize("rank", [0, 8])
def test_solve_reaches_tol_on_the_true_residual_up_to_the_operator_error(AGP, rank):
    tol = 1e-4
    X, y, K, b, _, _ = _dense(0)
    B = np.random.default_rng(rank).standard_normal((N, 3))
    res = {}
    for dtype in (np.float32, np.float64):
        m = _model(AGP, 0, rank, tol, dtype)
        x = m.solve(B).astype(R32.LD)
        info = m.info
        m.close()
        nb = np.sqrt(np.sum(B.astype(R32.LD) ** 2, axis=0))
        res[dtype] = np.sqrt(np.sum((B - K @ x) ** 2, axis=0)) / nb
        if dtype is np.float32:
            E = R32.bound(K, b, np.abs(x), K @ np.abs(x), True, False)
            allow = tol + (info["iterations"] + 1) * np.sqrt(np.sum(E ** 2, axis=0)) / nb
            assert info["converged"].all()
    print(f"true residual: Float32 operator {res[np.float32].astype(float)}, Float64 operator {res[np.float64].astype(float)}; "
          f"Float32 / bound {float(np.max(res[np.float32] / allow)):.2e}")
    assert np.all(res[np.float32] <= allow)


@pytest.mark.parametrize("kind,rank", [(0, 0), (1, 8), (2, 8)])
def test_likelihood_agrees_with_the_float64_operator_to_first_order(AGP, kind, rank):
    tol = 1e-10
    X, y, K, dK, Minv, cond = _dense(kind)
    out = {}
    for dtype in (np.float32, np.float64):
        m = _model(AGP, kind, rank, tol, dtype)
        m._solver()
        t = N + m.rank_used
        out[dtype] = m.log_marginal_likelihood(base_samples=np.sqrt(t) * np.eye(t), grad=True)
        assert m.info["converged"].all()
        m.close()
    a = Minv @ y
    # G = dM / d theta for (variance, scales[D], noise); scales: dK_ij / d s_d = phi'(d2) (2 / s) (s x_id - s x_jd)^2
    sx = (X * SCALE).astype(R32.LD)
    d2, _ = KR.distances(sx, sx)
    Gs = [K - R32.LD(NOISE) * np.eye(N)] + [GR.dphi(kind, d2)[0] * (2 / R32.LD(SCALE)) * (sx[:, None, d] - sx[None, :, d]) ** 2 for d in range(D)]
    Gs = [G.astype(np.float64) for G in Gs + [np.eye(N)]]
    first = lambda c, u, W: float(c * np.abs(u) @ dK @ np.abs(a) + 0.5 * np.sum(np.abs(W) * dK))  # noqa: E731
    ct, quad = 4 * cond * tol, 0.5 * 16 * _slq_deviation()[0]
    solve = lambda u, G: ct * (np.linalg.norm(a) * np.linalg.norm(u) + 0.5 * np.sqrt(np.trace(Minv) / NOISE) * np.linalg.norm(G))  # noqa: E731
    (v32, g32), (v64, g64) = out[np.float32], out[np.float64]
    bound_v = first(0.5, a, Minv) + 2 * (quad + 0.5 * ct * np.linalg.norm(y) * np.linalg.norm(a))
    flat = lambda g: np.array([g["variance"]] + list(g["scales"]) + [g["noise"]])  # noqa: E731
    bound_g = np.array([first(1.0, Minv @ (G @ a), Minv @ G @ Minv) + 2 * solve(G @ a, G) for G in Gs])
    diff = np.abs(flat(g32) - flat(g64))
    print(f"log p {v64:.6f} (Float64) {v32:.6f} (Float32), difference / bound {abs(v32 - v64) / bound_v:.2e}; gradient differences / "
          f"bounds {np.array2string(diff / bound_g, precision=2)}")
    assert abs(v32 - v64) <= bound_v and np.all(diff <= bound_g)
