"""`kernel_bilinear_grad` (csrc/agp_kmv_grad.h) against the dense long-double sums of tests/_kmv_grad_ref.py, inside that module's
budget, which is evaluated from the reference quantities alone."""
import numpy as np
import pytest

import _kmv_grad_ref as GR

pytestmark = pytest.mark.gpu
VARIANCE = 1.3
# (n, D, r, col_groups, kind, ard, every point twice)
CASES = [(1, 1, 1, 1, 0, False, False), (64, 16, 16, 1, 0, False, False), (65, 17, 17, 3, 1, True, False),
         (130, 33, 32, 3, 2, True, False), (130, 64, 40, 1, 0, True, False), (65, 64, 32, 3, 1, False, False),
         (130, 16, 1, 3, 2, False, False), (64, 1, 17, 1, 1, False, False), (130, 17, 40, 3, 0, False, False),
         (65, 33, 16, 1, 2, True, False), (130, 16, 32, 1, 0, False, True), (130, 64, 17, 3, 2, False, False),
         (1, 64, 32, 1, 1, True, False), (64, 33, 1, 3, 0, True, False), (65, 1, 40, 1, 2, False, False),
         (130, 16, 32, 3, 1, True, False), (130, 33, 17, 3, 1, False, True), (65, 16, 16, 3, 2, False, False),
         (130, 17, 32, 1, 2, True, False), (64, 64, 16, 1, 0, False, False)]


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _kernel(AGP, kind, scales, ard):
    k = [AGP.SqExponentialKernel, AGP.Matern52Kernel, AGP.Matern32Kernel][kind]()
    return VARIANCE * (k @ (AGP.ARDTransform(scales) if ard else AGP.ScaleTransform(scales[0])))


@pytest.mark.parametrize("n,D,r,groups,kind,ard,dup", CASES)
def test_against_the_dense_long_double_sums(AGP, n, D, r, groups, kind, ard, dup):
    rng = np.random.default_rng([n, D, r, kind])
    X = rng.random((n, D))
    if dup:
        X[n // 2:] = X[:n - n // 2]  # close-point repair and exact zeros off the diagonal
    scales = (np.geomspace(0.3, 3.0, D)[::-1].copy() if ard else np.full(D, 1.7)) / np.sqrt(D)  # d2 = O(1) at every D
    U, V, w = rng.standard_normal((n, r)), rng.standard_normal((n, r)), rng.standard_normal(r)
    dvar, dsc = AGP.kernel_bilinear_grad(_kernel(AGP, kind, scales, ard), X, U, V, w, col_groups=groups)
    rv, rs, bv, bs = GR.reference(kind, scales, VARIANCE, X, U, V, w)
    print(f"dvar error / bound {float(abs(dvar - rv) / bv):.2e}, worst dscale error / bound {float(np.max(np.abs(dsc - rs) / bs)):.2e}")
    assert abs(dvar - rv) <= bv and np.all(np.abs(dsc - rs) <= bs)
    again = AGP.kernel_bilinear_grad(_kernel(AGP, kind, scales, ard), X, U, V, w, col_groups=groups)
    assert again[0] == dvar and np.array_equal(again[1].view(np.int64), dsc.view(np.int64))


def test_exponential_kernel_is_refused_by_name(AGP):
    X = np.random.default_rng(0).random((5, 2))
    with pytest.raises(NotImplementedError, match="ExponentialKernel"):
        AGP.kernel_bilinear_grad(AGP.ExponentialKernel() @ AGP.ScaleTransform(1.0), X, X[:, :1], X[:, :1])
