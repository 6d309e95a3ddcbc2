"""The matrix-free kernel operator `agp_kernel_matmul` (csrc/agp_kmv.h): Out = (K(X, Y) + diag_add [X is Y]) V against a dense
np.longdouble kernel matrix built by direct differences (tests/_kmat_ref.py) and multiplied in long double.

Bound per output element (derived, not tuned), with b_ij = _kmat_ref.budget of the kernel value, R = r padded to 16, u = 2^-53:

    |Out_ic - ref_ic| <= sum_j ( b_ij |V_jc| + gamma_{p + R} |K_ij V_jc| )

the first term is the kernel values' own element-wise budget carried through the product, the second the MFMA dot product of length
p (tile by tile, in order) and the sum over at most 16 <= R column-group slices.
"""
import ctypes as C

import numpy as np
import pytest

import _kmat_ref as KR
from _pitched import Pitched

pytestmark = pytest.mark.gpu
LD = np.longdouble
VARIANCE = 1.3


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    yield dict(torch=torch, capi=capi, L=L, ctx=ctx)
    L.agp_ctx_destroy(ctx)


def _scales(D, ard):
    return np.geomspace(0.3, 3.0, D)[::-1].copy() if ard else np.full(D, 1.7)


def _desc(capi, kind, scales, ard):
    d = capi.KernelDesc()
    d.kind, d.variance, d.has_variance, d.has_transform, d.ard, d.scale = kind, VARIANCE, 1, 1, int(ard), float(scales[0])
    keep = (C.c_double * len(scales))(*scales)
    d.ard_scales_host = C.cast(keep, C.POINTER(C.c_double)) if ard else None
    return d, keep


def _call(env, kind, scales, ard, X, Y, V, diag_add=0.0, groups=0, pitch=0, D=None, r=None, ldv=None):
    """One call; Y=None is the symmetric form.  pitch > 0: every operand pitched by that many elements, base off alignment.
    Returns (status, the output canary)."""
    L, ctx = env["L"], env["ctx"]
    kd, keep = _desc(env["capi"], kind, scales, ard)
    mk = lambda a: Pitched("f64", data=a, ld=a.shape[1] + pitch, off=1 if pitch else 0, device="cuda")  # noqa: E731
    x, v, y = mk(X), mk(V), None if Y is None else mk(Y)
    out = Pitched("f64", rows=len(X), width=V.shape[1], ld=V.shape[1] + pitch, off=1 if pitch else 0, device="cuda")
    st = L.agp_kernel_matmul(ctx, 0, C.byref(kd), x.ptr, len(X), x.ld, None if y is None else y.ptr, len(V), 0 if y is None else y.ld,
                             X.shape[1] if D is None else D, int(Y is None), diag_add, v.ptr, v.ld if ldv is None else ldv,
                             V.shape[1] if r is None else r, groups, out.ptr, out.ld)
    out.check("out")
    return st, out


def _reference(kind, scales, X, Y, V, diag_add=0.0):
    """(Out in long double, the bound of the module docstring)"""
    D, r = X.shape[1], V.shape[1]
    d2, s2 = KR.distances(KR.scaled(X, scales, "f64"), KR.scaled(X if Y is None else Y, scales, "f64"))
    K = KR.reference(kind, "f64", VARIANCE, d2)
    if Y is None:
        K = K + LD(diag_add) * np.eye(len(X), dtype=LD)
    b = KR.budget(kind, "f64", D, VARIANCE, d2, s2)
    aV = np.abs(V.astype(LD))
    bound = b @ aV + KR.gamma(len(V) + (r + 15) // 16 * 16, KR.U["f64"]) * (np.abs(K) @ aV)
    return K @ V.astype(LD), bound, K


def _data(n, p, r, D, seed):
    """X, Y with every fifth row of Y a copy of, or a close neighbour of, a row of X (the repair of close points), V"""
    rng = np.random.default_rng([n, p, r, D, seed])
    X, Y = rng.random((n, D)), rng.random((p, D))
    for j in range(0, p, 5):
        Y[j] = X[(7 * j) % n] + (0.0 if j % 10 else 1e-7 * rng.standard_normal(D))
    return X, Y, rng.standard_normal((p, r))


# (n, p, r, D, kind, ard, col_groups): every listed n, p, r, D, the four kinds, both kinds of scale, groups 0 / 1 / 3 (3 at p = 200:
# four column tiles in groups of 2, 1, 1)
CASES = [(1, 1, 1, 1, 0, False, 0), (63, 64, 15, 3, 1, True, 1), (64, 65, 16, 33, 2, False, 0), (65, 200, 17, 64, 3, True, 3),
         (129, 200, 32, 3, 0, True, 3), (129, 65, 32, 64, 1, False, 0), (65, 1, 1, 33, 3, True, 1), (64, 200, 16, 1, 2, False, 0)]


@pytest.mark.parametrize("n,p,r,D,kind,ard,groups", CASES)
def test_product_within_the_derived_bound(env, n, p, r, D, kind, ard, groups):
    X, Y, V = _data(n, p, r, D, 0)
    sc = _scales(D, ard)
    st, out = _call(env, kind, sc, ard, X, Y, V, groups=groups)
    assert st == 0, env["L"].agp_last_error(env["ctx"])
    ref, bound, _ = _reference(kind, sc, X, Y, V)
    err = np.abs(out.window().astype(LD) - ref)
    print(f"worst error / bound {float(np.max(err / bound)):.3f}")
    assert not out.unwritten().any() and np.all(err <= bound)
    # a second call, pitched operands off alignment, and the same columns next to other neighbours: the same bits
    assert np.array_equal(_call(env, kind, sc, ard, X, Y, V, groups=groups)[1].bits(), out.bits())
    assert np.array_equal(_call(env, kind, sc, ard, X, Y, V, groups=groups, pitch=3)[1].bits(), out.bits())
    V2 = np.random.default_rng(1).standard_normal(V.shape)
    V2[:, r // 2] = V[:, r // 2]
    assert np.array_equal(_call(env, kind, sc, ard, X, Y, V2, groups=groups)[1].bits()[:, r // 2], out.bits()[:, r // 2])


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("form", ["sym", "drawn"])
def test_coincident_points_and_the_diagonal(env, kind, form):
    """n = 65, exact duplicate rows.  sym: Y is X, V = columns of the identity, so Out is K itself: the diagonal is exactly
    variance + diag_add, a duplicate pair exactly the variance.  drawn: Y = rows drawn from X, through the general form."""
    n, D, diag_add = 65, 3, 0.01
    rng = np.random.default_rng(5)
    X = 10.0 + rng.random((n, D))  # off the origin: the GEMM form of d2 cancels
    X[10], X[64] = X[3], X[0]
    sc = _scales(D, True)
    cols = np.r_[0:30, 63, 64]
    if form == "sym":
        V = np.eye(n)[:, cols]
        st, out = _call(env, kind, sc, True, X, None, V, diag_add=diag_add, groups=3)
        ref, bound, _ = _reference(kind, sc, X, None, V, diag_add)
        got = out.window()
        assert np.all(got[cols, np.arange(32)] == VARIANCE + diag_add)
        assert got[10, 3] == VARIANCE and got[3, 10] == VARIANCE and got[64, 0] == VARIANCE
    else:
        Y = X[rng.permutation(n)[:40]]
        V = rng.standard_normal((40, 7))
        st, out = _call(env, kind, sc, True, X, Y, V)
        ref, bound, _ = _reference(kind, sc, X, Y, V)
    assert st == 0, env["L"].agp_last_error(env["ctx"])
    assert np.all(np.abs(out.window().astype(LD) - ref) <= bound)


@pytest.mark.parametrize("change,status", [(dict(D=65), 5), (dict(r=33), 1), (dict(ldv=3), 1)])
def test_refused_with_outputs_untouched(env, change, status):
    X, Y, V = _data(20, 30, 4, 5, 0)
    if "D" in change:
        X, Y = np.ones((20, 65)), np.ones((30, 65))
    if "r" in change:
        V = np.ones((30, 33))
    st, out = _call(env, 0, _scales(X.shape[1], False), False, X, Y, V, **change)
    assert st == status and out.unwritten().all()
    assert b"agp_kernel_matmul" in env["L"].agp_last_error(env["ctx"])


def test_python_interface_takes_more_than_32_columns(env):
    import agp_amd as AGP

    X, Y, V = _data(65, 70, 40, 3, 2)
    k = VARIANCE * (AGP.Matern32Kernel() @ AGP.ScaleTransform(1.7))
    ref, bound, _ = _reference(2, _scales(3, False), X, Y, V)
    assert np.all(np.abs(AGP.kernel_matmul(k, X, V, Y=Y).astype(LD) - ref) <= bound)
