"""`kernel_matmul_grad` (csrc/agp_kmv_dx.h) against the dense long-double sums of tests/_kmv_dx_ref.py, inside that module's budget,
which is evaluated from the reference quantities alone."""
import ctypes as C

import numpy as np
import pytest

import _kmv_dx_ref as DR

pytestmark = pytest.mark.gpu
VARIANCE = 1.3
# (n, p, D, r, col_groups, kind, ard, paired, coincident: half of X copied from Y; "offset": the same with X, Y = 10 + U[0, 1))
CASES = [(1, 1, 1, 1, 1, 0, False, False, False), (63, 64, 16, 3, 1, 1, True, False, False), (65, 65, 17, 5, 3, 2, False, False, False),
         (129, 200, 33, 32, 3, 0, True, False, False), (65, 200, 64, 33, 1, 1, False, False, False),
         (129, 65, 64, 1, 3, 2, True, False, True), (63, 200, 16, 5, 3, 0, False, False, "offset"),
         (129, 64, 1, 3, 1, 1, False, False, False), (1, 200, 33, 32, 3, 2, True, False, False), (65, 1, 17, 1, 1, 0, True, False, False),
         (63, 65, 64, 5, 1, 0, True, False, False), (129, 200, 17, 33, 3, 1, True, False, False),
         (1, 65, 16, 1, 1, 0, False, True, False), (17, 200, 33, 17, 3, 1, True, True, True), (32, 64, 64, 32, 1, 2, False, True, False),
         (33, 200, 17, 33, 3, 0, True, True, False)]


@pytest.fixture(scope="module")
def AGP(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd

    return agp_amd


def _kernel(AGP, kind, scales, ard):
    k = [AGP.SqExponentialKernel, AGP.Matern52Kernel, AGP.Matern32Kernel, AGP.ExponentialKernel][kind]()
    return VARIANCE * (k @ (AGP.ARDTransform(scales) if ard else AGP.ScaleTransform(scales[0])))


def _inputs(n, p, D, r, kind, ard, coincident):
    rng = np.random.default_rng([n, p, D, r, kind])
    X, Y = rng.random((n, D)), rng.random((p, D))
    if coincident:
        X[:n // 2] = Y[:n // 2]  # t = 0: the close-point repair, and terms that must cancel in the expanded form
    if coincident == "offset":
        X, Y = X + 10.0, Y + 10.0
    scales = (np.geomspace(0.3, 3.0, D)[::-1].copy() if ard else np.full(D, 1.7)) / np.sqrt(D)  # d2 = O(1) at every D
    return X, Y, rng.standard_normal((p, r)), scales


@pytest.mark.parametrize("n,p,D,r,groups,kind,ard,paired,coincident", CASES)
def test_against_the_dense_long_double_sums(AGP, n, p, D, r, groups, kind, ard, paired, coincident):
    X, Y, V, scales = _inputs(n, p, D, r, kind, ard, coincident)
    k = _kernel(AGP, kind, scales, ard)
    out = AGP.kernel_matmul_grad(k, X, V, Y, paired=paired, col_groups=groups)
    ref, bound = DR.reference(kind, scales, VARIANCE, X, Y, V, paired, groups)
    assert out.shape == ref.shape
    print(f"worst error / bound {float(np.max(np.abs(out - ref) / bound)):.2e}")
    assert np.all(np.abs(out - ref) <= bound)
    again = AGP.kernel_matmul_grad(k, X, V, Y, paired=paired, col_groups=groups)
    assert np.array_equal(again.view(np.int64), out.view(np.int64))


def test_a_column_depends_on_its_own_column_of_V_only(AGP):
    X, Y, V, scales = _inputs(65, 65, 17, 5, 2, False, False)
    k = _kernel(AGP, 2, scales, False)
    out = AGP.kernel_matmul_grad(k, X, V, Y, col_groups=3)
    V2 = V.copy()
    V2[:, [0, 1, 3, 4]] *= -7.5  # the other columns of its block of 4, and the next block
    out2 = AGP.kernel_matmul_grad(k, X, V2, Y, col_groups=3)
    assert np.array_equal(out2[:, 2].view(np.int64), out[:, 2].view(np.int64)) and not np.array_equal(out2[:, 3], out[:, 3])


@pytest.mark.parametrize("what,status", [("exponential", 5), ("D65", 5), ("paired", 1)])
def test_refusals(AGP, what, status):
    import torch
    from agp_amd import capi, iterative

    n, p, D, r = 4, 6, 65 if what == "D65" else 3, 3
    X, Y, V = np.ones((n, D)), np.ones((p, D)), np.ones((p, r))
    k = _kernel(AGP, 3 if what == "exponential" else 0, np.ones(D), False)
    if what == "exponential":
        with pytest.raises(NotImplementedError, match="ExponentialKernel"):
            AGP.kernel_matmul_grad(k, X, V, Y)
    cx = iterative._Ctx()
    x, y, v = cx.dev_tensor(X), cx.dev_tensor(Y), cx.dev_tensor(V)
    out = torch.full((n, r * D), 7.0, dtype=torch.float64, device=cx.dev)
    kd, keep = k.desc(D)
    st = capi.lib().agp_kernel_matmul_dx(cx.ctx, capi.F64, C.byref(kd), x.data_ptr(), n, D, y.data_ptr(), p, D, D, v.data_ptr(), r, r,
                                         1 if what == "paired" else 0, 0, out.data_ptr(), r * D)
    assert st == status and bool((out == 7.0).all())  # refused before the caller's buffer is touched
    with pytest.raises(capi.AGPError, match="ExponentialKernel" if what == "exponential" else "D <= 64" if what == "D65" else "paired"):
        cx.chk(st)
    cx.close()
