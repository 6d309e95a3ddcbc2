"""The wide block of the matrix-free kernel operator (`agp_kernel_matmul_wide`, csrc/agp_kmv_wide.h; `kernel_matmul(block=128)`): up to
128 columns of V per launch.  Data, long-double reference and bound are those of tests/test_gpu_kernel_matmul.py (its `_data`,
`_reference`: |V|'b + gamma_{p + R} |K||V|, R the columns padded to 16 -- computed here per block of 128 columns, never wider than
that file's own).  On top of the bound: the same k-step order makes every column equal `block=32`'s bit for bit.
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


def _kernel(AGP, kind, D, ard):
    tr = AGP.ARDTransform(T._scales(D, True)) if ard else AGP.ScaleTransform(1.7)
    return T.VARIANCE * (getattr(AGP, KINDS[kind])() @ tr)


# (n, p, r, D, kind, ard, col_groups, sym): every listed n, p, D and r once (33 .. 48, 49 .. 64, 65 .. 96, 97 .. 128 are the four
# instances; 129 is a block of 128 and a block of 1), the four kinds, groups 0 / 1 / 3, both forms (sym: p = n)
CASES = [(1, 1, 33, 1, 0, False, 0, False), (63, 64, 48, 17, 1, True, 1, False), (65, 65, 49, 33, 2, False, 0, False),
         (129, 200, 64, 64, 3, True, 3, False), (65, 200, 65, 17, 0, True, 3, False), (63, 65, 96, 64, 1, False, 0, False),
         (129, 64, 97, 1, 2, True, 1, False), (65, 200, 128, 64, 0, False, 3, False), (129, 200, 128, 33, 3, False, 0, False),
         (63, 1, 129, 17, 1, True, 0, False), (129, 129, 129, 64, 2, True, 3, True), (65, 65, 128, 33, 1, True, 3, True),
         (1, 1, 48, 1, 3, False, 0, True)]


@pytest.mark.parametrize("n,p,r,D,kind,ard,groups,sym", CASES)
def test_within_the_bound_and_bit_for_bit_the_32_column_path(env, n, p, r, D, kind, ard, groups, sym):  # noqa: F811
    import agp_amd as AGP

    X, Y, V = T._data(n, p, r, D, 0)
    Y, diag_add = (None, 0.01) if sym else (Y, 0.0)
    k = _kernel(AGP, kind, D, ard)
    wide = AGP.kernel_matmul(k, X, V, Y=Y, diag_add=diag_add, col_groups=groups, block=128)  # (a TypeError before the wide block)
    worst = 0.0
    for c0 in range(0, r, 128):
        ref, bound, _ = T._reference(kind, T._scales(D, ard), X, Y, V[:, c0:c0 + 128], diag_add)
        err = np.abs(wide[:, c0:c0 + 128].astype(LD) - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
    print(f"worst error / bound {worst:.3f}")
    narrow = AGP.kernel_matmul(k, X, V, Y=Y, diag_add=diag_add, col_groups=groups, block=32)
    assert np.array_equal(wide.view(np.int64), narrow.view(np.int64))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_exact_diagonal_with_duplicate_rows(env, kind):  # noqa: F811
    """n = 65, V = I (65 columns, the instance of 96), duplicate rows: Out is K itself, its diagonal exactly variance + diag_add"""
    import agp_amd as AGP

    n, D, diag_add = 65, 3, 0.01
    X = 10.0 + np.random.default_rng(5).random((n, D))
    X[10], X[64] = X[3], X[0]
    got = AGP.kernel_matmul(_kernel(AGP, kind, D, True), X, np.eye(n), diag_add=diag_add, col_groups=3, block=128)
    assert np.all(np.diag(got) == T.VARIANCE + diag_add)
    assert got[10, 3] == T.VARIANCE and got[3, 10] == T.VARIANCE and got[64, 0] == T.VARIANCE
    ref, bound, _ = T._reference(kind, T._scales(D, True), X, None, np.eye(n), diag_add)
    assert np.all(np.abs(got.astype(LD) - ref) <= bound)


@pytest.mark.parametrize("D,r,dtype,status", [(5, 129, 0, 1), (65, 40, 0, 5), (5, 40, 1, 5)])
def test_refused_by_name_with_outputs_untouched(env, D, r, dtype, status):  # noqa: F811
    L, ctx = env["L"], env["ctx"]
    kd, keep = T._desc(env["capi"], 0, T._scales(D, False), False)
    x, y, v = (Pitched("f64", data=np.ones(s), device="cuda") for s in ((20, D), (30, D), (30, r)))
    out = Pitched("f64", rows=20, width=r, device="cuda")
    st = L.agp_kernel_matmul_wide(ctx, dtype, C.byref(kd), x.ptr, 20, x.ld, y.ptr, 30, y.ld, D, 0, 0.0, v.ptr, v.ld, r, 0, out.ptr, out.ld)
    out.check("out")
    assert st == status and out.unwritten().all()
    assert b"agp_kernel_matmul_wide" in L.agp_last_error(ctx)


def test_other_blocks_are_refused(env):  # noqa: F811
    import agp_amd as AGP

    with pytest.raises(ValueError, match="block must be 32 or 128"):
        AGP.kernel_matmul(_kernel(AGP, 0, 3, False), np.ones((4, 3)), np.ones((4, 2)), block=64)
