"""The Float32 kernel operator (csrc/agp_kmv_f32.h) against a dense np.longdouble kernel matrix by direct differences from the inputs as
given, multiplied in long double, within the derived bound of tests/_kmv32_ref.py.  Float32 storage is `agp_kernel_matmul(AGP_F32)`;
Float64 storage of V and Out is the solver handle's operator (`agp_gp_cg_set_operator_dtype` + `agp_gp_cg_apply`: symmetric, diag_add =
sigma2).  Data: 10 + U[0, 1) in Float32, every fifth row of Y (of X in the symmetric form) a copy or a 1e-4 neighbour of a row of X."""
import ctypes as C

import numpy as np
import pytest

import _kmv32_ref as R32
from _pitched import Pitched
from test_gpu_kernel_matmul import VARIANCE, _desc, _scales, env  # noqa: F401

pytestmark = pytest.mark.gpu
LD = np.longdouble
DIAG = 0.01
P_WIN = 64 * R32.F + 65  # crosses a flush window by one tile and one column


def _call(env, kind, sc, ard, X, Y, V, store, groups=0, pitch=0, D=None, r=None, ldv=None, dtype=1):
    """One product; Y=None is the symmetric form with diag_add = DIAG.  Returns (status, the output canary)."""
    L, ctx = env["L"], env["ctx"]
    kd, keep = _desc(env["capi"], kind, sc, ard)
    mk = lambda a: Pitched(store, data=a, ld=a.shape[1] + pitch, off=1 if pitch else 0, device="cuda")  # noqa: E731
    x, v, y = mk(X), mk(V), None if Y is None else mk(Y)
    out = Pitched(store, rows=len(X), width=V.shape[1], ld=V.shape[1] + pitch, off=1 if pitch else 0, device="cuda")
    n, rr = len(X), V.shape[1] if r is None else r
    if store == "f32":
        st = L.agp_kernel_matmul(ctx, dtype, C.byref(kd), x.ptr, n, x.ld, None if y is None else y.ptr, len(V), 0 if y is None else y.ld,
                                 X.shape[1] if D is None else D, int(Y is None), DIAG, v.ptr, v.ld if ldv is None else ldv, rr, groups,
                                 out.ptr, out.ld)
    else:
        h = C.c_void_p()
        assert L.agp_gp_cg_create(ctx, C.byref(kd), x.ptr, n, x.ld, X.shape[1], DIAG, 0, C.byref(h), None) == 0
        assert L.agp_gp_cg_set_operator_dtype(h, 1) == 0
        st = L.agp_gp_cg_apply(h, v.ptr, v.ld, rr, out.ptr, out.ld)
        L.agp_gp_cg_destroy(h)
    out.check("out")
    return st, out


def _data(n, p, r, D, sym, store):
    rng = np.random.default_rng([n, p, r, D])
    X = (10.0 + rng.random((n, D))).astype(np.float32)
    Y = X if sym else (10.0 + rng.random((p, D))).astype(np.float32)
    for j in range(0, p, 5):
        Y[j] = X[(7 * j + 1) % n] + (0.0 if j % 10 else 1e-4 * rng.standard_normal(D))
    if sym and n > 1:
        X[n - 1] = X[0]
    V = rng.standard_normal((p, r))
    return X, (None if sym else Y), (V.astype(np.float32) if store == "f32" else V)


# (n, p, r, D, kind, ard, col_groups, symmetric, storage of V and Out)
CASES = [(1, 1, 1, 1, 0, False, 0, False, "f32"), (63, 64, 15, 3, 1, True, 1, False, "f32"), (64, 65, 16, 33, 2, False, 0, False, "f32"),
         (65, P_WIN, 17, 64, 3, True, 3, False, "f32"), (129, P_WIN, 32, 17, 0, True, 3, False, "f32"),
         (129, 129, 32, 64, 1, False, 0, True, "f32"), (63, 63, 17, 17, 0, True, 3, True, "f32"), (65, 65, 1, 33, 3, True, 0, True, "f64"),
         (P_WIN, P_WIN, 16, 1, 2, False, 0, True, "f64"), (129, 129, 32, 3, 0, False, 0, True, "f64")]


@pytest.mark.parametrize("n,p,r,D,kind,ard,groups,sym,store", CASES)
def test_product_within_the_derived_bound(env, n, p, r, D, kind, ard, groups, sym, store):
    X, Y, V = _data(n, p, r, D, sym, store)
    sc = _scales(D, ard)
    run = lambda V, **kw: _call(env, kind, sc, ard, X.astype(V.dtype), None if sym else Y.astype(V.dtype), V, store, groups=groups, **kw)  # noqa: E731
    st, out = run(V)
    assert st == 0, env["L"].agp_last_error(env["ctx"])
    K, b = R32.operator(kind, sc, VARIANCE, X, Y, DIAG if sym else 0.0)
    ref = K @ V.astype(LD)
    err, bound = np.abs(out.window().astype(LD) - ref), R32.bound(K, b, V, ref, store == "f64", store == "f32")
    print(f"worst error / bound {float(np.max(err / bound)):.2e}")
    assert not out.unwritten().any() and np.all(err <= bound)
    # a second call, pitched operands off alignment, and the same column next to other neighbours: the same bits
    assert np.array_equal(run(V)[1].bits(), out.bits())
    assert np.array_equal(run(V, pitch=3)[1].bits(), out.bits())
    V2 = np.random.default_rng(1).standard_normal(V.shape).astype(V.dtype)
    V2[:, r // 2] = V[:, r // 2]
    assert np.array_equal(run(V2)[1].bits()[:, r // 2], out.bits()[:, r // 2])
    if sym and n > 1:  # K itself through columns of the identity: the diagonal and the duplicate pair (0, n - 1), in the output type
        got = run(np.eye(n, dtype=V.dtype)[:, :r])[1].window()
        var = np.float64(np.float32(VARIANCE))
        assert np.all(np.diag(got) == V.dtype.type(var + DIAG)) and got[n - 1, 0] == V.dtype.type(var)


@pytest.mark.parametrize("change,status", [(dict(D=65), 5), (dict(r=33), 1), (dict(ldv=3), 1), (dict(dtype=7), 1)])
def test_refused_with_outputs_untouched(env, change, status):
    X, Y, V = _data(20, 30, 4, 5, False, "f32")
    if "D" in change:
        X, Y = np.ones((20, 65), np.float32), np.ones((30, 65), np.float32)
    if "r" in change:
        V = np.ones((30, 33), np.float32)
    st, out = _call(env, 0, _scales(X.shape[1], False), False, X, Y, V, "f32", **change)
    assert st == status and out.unwritten().all()
    assert b"agp_kernel_matmul" in env["L"].agp_last_error(env["ctx"])


def test_python_interface_converts_and_takes_more_than_32_columns(env):
    import agp_amd as AGP

    X, Y, V = _data(65, 70, 40, 3, False, "f32")
    K, b = R32.operator(2, _scales(3, False), VARIANCE, X, Y)
    k, ref = VARIANCE * (AGP.Matern32Kernel() @ AGP.ScaleTransform(1.7)), K @ V.astype(LD)
    got = AGP.kernel_matmul(k, X.astype(np.float64), V.astype(np.float64), Y=Y.astype(np.float64), dtype=np.float32)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(LD) - ref) <= R32.bound(K, b, V, ref, False, True))
