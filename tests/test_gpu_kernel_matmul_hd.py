"""The matrix-free kernel operator for 65 .. 128 input dimensions (`agp_kernel_matmul_hd`, csrc/agp_kmv_hd.h), through
`kernel_matmul`.  Data, long-double reference and bound are those of tests/test_gpu_kernel_matmul.py (`_data`, `_reference`:
|V|'b + gamma_{p + R} |K||V| with b = _kmat_ref.budget, a function of D), per block of 32 columns.  The scales are that file's times
sqrt(3 / D): the typical scaled squared distance is then what it is at D = 3, and the kernel values are not all but zero.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_kernel_matmul as T
from _pitched import Pitched
from test_gpu_kernel_matmul import env  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble
KINDS = ["SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel"]


def _scales(D, ard):
    return T._scales(D, ard) * np.sqrt(3.0 / D)


def _kernel(AGP, kind, sc, ard):
    return T.VARIANCE * (getattr(AGP, KINDS[kind])() @ (AGP.ARDTransform(sc) if ard else AGP.ScaleTransform(float(sc[0]))))


def _check(got, kind, sc, X, Y, V, diag_add):
    """every block of 32 columns inside the bound; returns the reference kernel matrix"""
    for c0 in range(0, V.shape[1], 32):
        ref, bound, K = T._reference(kind, sc, X, Y, V[:, c0:c0 + 32], diag_add)
        err = np.abs(got[:, c0:c0 + 32].astype(LD) - ref)
        print(f"columns {c0}..: worst error / bound {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound)
    return K


# (n, p, r, D, kind, ard, col_groups, sym): every listed n, p, r (40: two blocks) and D (65 and 96: the instance of 96 at both ends,
# 97 and 128: that of 128) once, the four kinds, both kinds of scale, groups 0 / 1 / 3 (3 at p = 200 and in one sym case), both forms
CASES = [(1, 1, 1, 65, 0, False, 0, False), (63, 64, 16, 96, 1, True, 1, False), (65, 65, 17, 97, 2, False, 0, True),
         (129, 200, 32, 128, 3, True, 3, False), (65, 200, 40, 65, 0, True, 3, False), (129, 129, 40, 128, 1, False, 3, True),
         (63, 1, 16, 97, 3, False, 0, False), (129, 64, 1, 96, 2, True, 1, False)]


@pytest.mark.parametrize("n,p,r,D,kind,ard,groups,sym", CASES)
def test_product_within_the_derived_bound(env, n, p, r, D, kind, ard, groups, sym):  # noqa: F811
    import agp_amd as AGP

    X, Y, V = T._data(n, p, r, D, 0)
    Y, diag_add = (None, 0.01) if sym else (Y, 0.0)
    sc = _scales(D, ard)
    k = _kernel(AGP, kind, sc, ard)
    got = AGP.kernel_matmul(k, X, V, Y=Y, diag_add=diag_add, col_groups=groups)  # (AGPError at D = 65 before k_kmv_hd)
    K = _check(got, kind, sc, X, Y, V, diag_add)
    # the case tests more than the diagonal: the typical kernel value (planted copies and the diagonal aside) is neither 0 nor 1
    free = np.ones(K.shape, dtype=bool)
    if sym:
        np.fill_diagonal(free, False)
    else:
        free[(7 * np.arange(0, p, 5)) % n, np.arange(0, p, 5)] = False
    assert not free.any() or 0.05 < float(np.median(K[free])) / T.VARIANCE < 0.9
    # a second call, and the same column next to other neighbours: the same bits
    assert np.array_equal(AGP.kernel_matmul(k, X, V, Y=Y, diag_add=diag_add, col_groups=groups).view(np.int64), got.view(np.int64))
    V2 = np.random.default_rng(1).standard_normal(V.shape)
    V2[:, r // 2] = V[:, r // 2]
    got2 = AGP.kernel_matmul(k, X, V2, Y=Y, diag_add=diag_add, col_groups=groups)
    assert np.array_equal(got2[:, r // 2].view(np.int64), got[:, r // 2].view(np.int64))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_exact_diagonal_with_duplicate_rows(env, kind):  # noqa: F811
    """n = 65, V = I, duplicate rows far from the origin: Out is K itself, its diagonal exactly variance + diag_add, a duplicate pair
    exactly the variance (the repair reads whole rows from global memory and reproduces the fragments' values)"""
    import agp_amd as AGP

    n, D, diag_add = 65, 65, 0.01
    X = 10.0 + np.random.default_rng(5).random((n, D))
    X[10], X[64] = X[3], X[0]
    sc = _scales(D, True)
    got = AGP.kernel_matmul(_kernel(AGP, kind, sc, True), X, np.eye(n), diag_add=diag_add, col_groups=3)
    assert np.all(np.diag(got) == T.VARIANCE + diag_add)
    assert got[10, 3] == T.VARIANCE and got[3, 10] == T.VARIANCE and got[64, 0] == T.VARIANCE and got[0, 64] == T.VARIANCE
    _check(got, kind, sc, X, None, np.eye(n), diag_add)


@pytest.mark.parametrize("D,dtype,status", [(64, 0, 1), (129, 0, 5), (96, 1, 5)])
def test_refused_by_name_with_outputs_untouched(env, D, dtype, status):  # noqa: F811
    L, ctx = env["L"], env["ctx"]
    kd, keep = T._desc(env["capi"], 0, _scales(D, False), False)
    x, y, v = (Pitched("f64", data=np.ones(s), device="cuda") for s in ((20, D), (30, D), (30, 4)))
    out = Pitched("f64", rows=20, width=4, device="cuda")
    st = L.agp_kernel_matmul_hd(ctx, dtype, C.byref(kd), x.ptr, 20, x.ld, y.ptr, 30, y.ld, D, 0, 0.0, v.ptr, v.ld, 4, 0, out.ptr, out.ld)
    out.check("out")
    assert st == status and out.unwritten().all()
    assert b"agp_kernel_matmul_hd" in L.agp_last_error(ctx)
