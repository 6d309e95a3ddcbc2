"""Greedy conditional-variance selection on the device (`agp_greedy_variance`, csrc/agp_greedy.h; `ConditionalVariance`) against the
NumPy restatement tests/_greedy_ref.py.

Parity bound.  The parity cases meet a margin condition (tests/test_greedy_host.py): every argmax after the first is decided by
>= 1e-6 relative and every pivot is >= 1e-6 variance, device and host arithmetic differ by far less, so the INDICES must be identical.
Factor and residual trace are held to 1e-9 * variance absolute: the accumulated error of a column is about
m * eps * variance / sqrt(smallest pivot) -- with m = 130, eps = 1.1e-16 and the smallest pivot 4e-6 that is 7e-12 * variance, so the
bound leaves two orders of margin.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

import _greedy_ref as G
import _kmat_ref as KR
from _pitched import Pitched, layouts

pytestmark = pytest.mark.gpu

INVALID = 1
NPT = {"f64": np.float64, "f32": np.float32}
DT = {"f64": 0, "f32": 1}


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


def _desc(capi, c):
    """(KernelDesc, keepalive) of a case dict (kind, scale or ARD scales, variance)."""
    d = capi.KernelDesc()
    d.kind, d.variance, d.has_variance, d.has_transform = G.KIND_ID[c["kind"]], c["variance"], 1, 1
    keep = None
    if np.ndim(c["scale"]):
        keep = (C.c_double * len(c["scale"]))(*c["scale"])
        d.ard, d.scale, d.ard_scales_host = 1, 1.0, C.cast(keep, C.POINTER(C.c_double))
    else:
        d.ard, d.scale, d.ard_scales_host = 0, c["scale"], None
    return d, keep


def _run(env, c, X, m, tol=1e-9, dtype="f64", factor=True):
    """One contiguous call; outputs pre-filled with NaN / a sentinel so that anything left unwritten shows."""
    torch, L, ctx = env["torch"], env["L"], env["ctx"]
    kd, keep = _desc(env["capi"], c)
    Xd = torch.as_tensor(np.ascontiguousarray(X, dtype=NPT[dtype])).cuda()
    N, D = Xd.shape
    idx = torch.full((m,), 12345, dtype=torch.int64, device="cuda")
    Z = torch.full((m, D), float("nan"), dtype=Xd.dtype, device="cuda")
    F = torch.full((N, m), float("nan"), dtype=torch.float64, device="cuda") if factor else None
    tr = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    nsel = C.c_int64(-7)
    st = L.agp_greedy_variance(ctx, DT[dtype], C.byref(kd), Xd.data_ptr(), N, D, D, m, tol, idx.data_ptr(), Z.data_ptr(), D,
                               F.data_ptr() if factor else None, m, tr.data_ptr(), C.byref(nsel))
    assert st == 0, L.agp_last_error(ctx)
    return dict(indices=idx.cpu().numpy(), Z=Z.cpu().numpy(), factor=F.cpu().numpy() if factor else None, trace=tr.cpu().numpy(),
                selected=int(nsel.value))


_device = {}


def _case(env, case):
    """The device result of a named case, computed once and shared (read-only)."""
    if case not in _device:
        c = G.CASES[case]
        _device[case] = _run(env, c, G.case_data(case), c["m"])
    return _device[case]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


@pytest.mark.parametrize("case", list(G.CASES))
def test_parity_with_the_restatement(env, case):
    c = G.CASES[case]
    X, ref = G.case_result(case)
    got = _case(env, case)
    assert got["selected"] == c["m"] == ref["selected"]
    assert np.array_equal(got["indices"], ref["indices"])
    ef = np.max(np.abs(got["factor"] - ref["factor"])) / c["variance"]
    et = np.max(np.abs(got["trace"] - ref["trace"])) / c["variance"]
    print(f"{case}: worst |factor - ref| {ef:.2e} variance, worst |trace - ref| {et:.2e} variance (bound 1e-9)")
    assert ef <= 1e-9 and et <= 1e-9
    assert np.array_equal(_bits(got["Z"]), _bits(X[ref["indices"]]))  # the chosen rows, bit copies


@pytest.mark.parametrize("case", list(G.CASES))
def test_first_column_against_the_kernel_matrix_kernel(env, case):
    """l_0 = k(X, x_0) / sqrt(variance): column 0 times sqrt(variance) is a column of agp_kernelmatrix, within the element-wise
    budget of DESIGN.md section 4a (tests/_kmat_ref.py)."""
    torch, L, ctx = env["torch"], env["L"], env["ctx"]
    c = G.CASES[case]
    X = np.array(G.case_data(case))
    got = _case(env, case)
    kd, keep = _desc(env["capi"], c)
    Xd = torch.as_tensor(X).cuda()
    out = torch.full((c["N"], 1), float("nan"), dtype=torch.float64, device="cuda")
    assert L.agp_kernelmatrix(ctx, 0, C.byref(kd), Xd.data_ptr(), c["N"], c["D"], None, Xd.data_ptr(), 1, c["D"], c["D"],
                              out.data_ptr(), 1) == 0, L.agp_last_error(ctx)
    col = out.cpu().numpy()[:, 0]
    mine = got["factor"][:, 0] * np.sqrt(c["variance"])
    sx = KR.scaled(X, c["scale"], "f64")
    d2, s2 = KR.distances(sx, sx[:1])
    b = np.asarray(KR.budget(G.KIND_ID[c["kind"]], "f64", c["D"], c["variance"], d2, s2), dtype=np.float64)[:, 0]
    worst = np.max(np.abs(mine - col) / b)
    print(f"{case}: worst |l_0 sqrt(variance) - K[:, 0]| / budget = {worst:.3f}")
    assert worst <= 1.0


def test_same_call_twice_is_bit_identical(env):
    c = G.CASES["sqexp_d3"]
    a = _case(env, "sqexp_d3")
    b = _run(env, c, G.case_data("sqexp_d3"), c["m"])
    for key in ("indices", "Z", "factor", "trace"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    assert a["selected"] == b["selected"]


def test_shorter_call_is_a_prefix(env):
    c = G.CASES["sqexp_d3"]
    a = _case(env, "sqexp_d3")
    b = _run(env, c, G.case_data("sqexp_d3"), 64)
    assert np.array_equal(b["indices"], a["indices"][:64])
    assert np.array_equal(_bits(b["factor"]), _bits(a["factor"][:, :64]))
    assert np.array_equal(_bits(b["trace"]), _bits(a["trace"][:64]))


@pytest.mark.parametrize("case,dtype", [("matern52_ard_d3", "f64"), ("sqexp_d33", "f64"), ("matern32_d1", "f32")])
def test_pitched_buffers_with_guard_bands(env, case, dtype):
    """x, z_out and factor_out with leading dimensions wider than their rows and bases off alignment, NaN guard bands everywhere
    outside the windows: bit-identical to the contiguous call, the guards untouched; idx_out / trace_out with guards at their ends."""
    L, ctx = env["L"], env["ctx"]
    c = G.CASES[case]
    N, D, m = c["N"], c["D"], c["m"]
    X = G.case_data(case).astype(NPT[dtype])
    ref = _run(env, c, X, m, dtype=dtype)
    kd, keep = _desc(env["capi"], c)
    for k in range(3):
        for off in (0, 1):
            def mk(dt, w, **kw):
                ld = [ld for ld, o in layouts(w, dt) if o == 0][k]
                return Pitched(dt, ld=ld, off=off, device="cuda", **kw)

            x = mk(dtype, D, data=X)
            z = mk(dtype, D, rows=m, width=D)
            f = mk("f64", m, rows=N, width=m)
            ix = Pitched("i64", rows=1, width=m, guard=1, device="cuda")
            tr = Pitched("f64", rows=1, width=m, guard=1, device="cuda")
            nsel = C.c_int64(-7)
            st = L.agp_greedy_variance(ctx, DT[dtype], C.byref(kd), x.ptr, N, x.ld, D, m, 1e-9, ix.ptr, z.ptr, z.ld, f.ptr, f.ld,
                                       tr.ptr, C.byref(nsel))
            tag = (case, dtype, k, off)
            assert st == 0, (tag, L.agp_last_error(ctx))
            for p in (x, z, f, ix, tr):
                p.check(str(tag))
                assert p is x or not p.unwritten().any(), tag
            assert nsel.value == m
            assert np.array_equal(ix.window()[0], ref["indices"]), tag
            assert np.array_equal(z.bits(), _bits(ref["Z"])), tag
            assert np.array_equal(f.bits(), _bits(ref["factor"])), tag
            assert np.array_equal(tr.bits()[0], _bits(ref["trace"])), tag


def test_f32_input_is_widened_on_load(env):
    c = G.CASES["sqexp_d3"]
    X32 = G.case_data("sqexp_d3").astype(np.float32)
    a = _run(env, c, X32, c["m"], dtype="f32")
    b = _run(env, c, X32.astype(np.float64), c["m"], dtype="f64")
    assert np.array_equal(a["indices"], b["indices"])
    assert np.array_equal(_bits(a["factor"]), _bits(b["factor"])) and np.array_equal(_bits(a["trace"]), _bits(b["trace"]))
    assert a["Z"].dtype == np.float32 and np.array_equal(_bits(a["Z"]), _bits(X32[a["indices"]]))


def test_early_stop_on_tiled_points(env):
    import agp_amd as AGP

    c = dict(kind="sqexponential", scale=2.0, variance=1.5)
    X = G.tiled_data()
    ref = G.greedy(G.case_kernel(c), X, 64, tol=1e-9)
    got = _run(env, c, X, 64, tol=1e-9)
    k = got["selected"]
    assert k == 40 == ref["selected"]
    assert sorted((got["indices"][:k] % 40).tolist()) == list(range(40))
    assert np.all(got["indices"][k:] == -1)
    assert np.all(got["factor"][:, k:] == 0.0) and np.all(got["trace"][k:] == 0.0) and np.all(got["Z"][k:] == 0.0)
    assert np.array_equal(_bits(got["Z"][:k]), _bits(X[got["indices"][:k]]))
    assert np.all(np.isfinite(got["factor"])) and np.all(np.isfinite(got["trace"]))
    kern = 1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0))
    with pytest.warns(UserWarning, match="selected 40 of the 64"):
        Z, info = AGP.inducingpoints(AGP.ConditionalVariance(64, kern, tol=1e-9), X, return_info=True)
    assert Z.shape == (40, 3) and Z.dtype == np.float64 and info["selected"] == 40 and info["factor"] is None
    assert np.array_equal(info["indices"], got["indices"][:40]) and np.array_equal(Z, X[info["indices"]])
    assert np.array_equal(_bits(info["trace"]), _bits(got["trace"][:40]))


def test_refusals_leave_the_outputs_untouched(env):
    torch, L, ctx, capi = env["torch"], env["L"], env["ctx"], env["capi"]
    c = G.CASES["sqexp_d3"]
    N, D, m = 50, 3, 8
    X = G.case_data("sqexp_d3")[:N]
    Xd = torch.as_tensor(X).cuda()
    ard = dict(c, scale=(1.0, 2.0, 3.0))
    good = dict(dtype=0, c=c, n=N, ldx=D, D=D, m=m, tol=1e-9, ldz=D, ldf=m)
    bad = [dict(n=0), dict(n=-1), dict(m=0), dict(m=-2), dict(m=N + 1), dict(D=0), dict(D=129, ldx=129, ldz=129), dict(ldx=D - 1),
           dict(ldz=D - 1), dict(ldf=m - 1), dict(tol=-1e-12), dict(tol=float("nan")), dict(dtype=2),
           dict(c=dict(c, kind=None)), dict(c=dict(c, variance=0.0)), dict(c=dict(c, variance=float("nan"))),
           dict(c=dict(c, scale=0.0)), dict(c=dict(ard, scale=(1.0, -2.0, 3.0))), dict(c=ard, null_ard=True), dict(null_k=True)]
    idx = Pitched("i64", rows=1, width=m, guard=1, device="cuda")
    z = Pitched("f64", rows=m, width=D, device="cuda")
    f = Pitched("f64", rows=N, width=m, device="cuda")
    tr = Pitched("f64", rows=1, width=m, guard=1, device="cuda")
    for change in bad:
        a = dict(good, **{k: v for k, v in change.items() if not k.startswith("null")})
        cc = a["c"]
        if cc["kind"] is None:
            kd, keep = _desc(capi, dict(cc, kind="sqexponential"))
            kd.kind = 4
        else:
            kd, keep = _desc(capi, cc)
        if change.get("null_ard"):
            kd.ard_scales_host = None
        nsel = C.c_int64(-7)
        st = L.agp_greedy_variance(ctx, a["dtype"], None if change.get("null_k") else C.byref(kd), Xd.data_ptr(), a["n"], a["ldx"],
                                   a["D"], a["m"], a["tol"], idx.ptr, z.ptr, a["ldz"], f.ptr, a["ldf"], tr.ptr, C.byref(nsel))
        assert st == INVALID, (change, st)
        assert nsel.value == -7, change
        for p in (idx, z, f, tr):
            assert p.unwritten().all(), change
            p.check(str(change))
    # the context stays usable
    got = _run(env, c, X, m)
    ref = G.greedy(G.case_kernel(c), X, m)
    assert np.array_equal(got["indices"], ref["indices"])


def test_end_to_end_svgp_on_the_selected_points(env):
    import agp_amd as AGP

    c = G.CASES["sqexp_d3"]
    X, y = G.e2e_data()
    kern = c["variance"] * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(c["scale"]))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        Z, info = AGP.inducingpoints(AGP.ConditionalVariance(64, kern), X, return_info=True)
    assert not [w for w in caught if "ConditionalVariance" in str(w.message)]  # 64 of 64: no early-stop warning
    assert Z.shape == (64, 3) and info["selected"] == 64 and np.array_equal(Z, X[info["indices"]])
    model = AGP.SVGP(kern, AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z, optimiser=False)
    AGP.train_(model, X, y, 20)
    elbo = AGP.ELBO(model, X, y)
    assert np.isfinite(elbo)
    Zr = AGP.inducingpoints(AGP.RandomSubset(64), X, rng=np.random.default_rng(0))
    ridx = [int(np.flatnonzero((X == zr).all(axis=1))[0]) for zr in Zr]
    rtrace = G.subset_trace(G.case_kernel(c), X, ridx)
    print(f"ELBO {elbo:.4f}; residual trace: ConditionalVariance(64) {info['trace'][-1]:.4e}, RandomSubset(64) {rtrace:.4e}")
    assert info["trace"][-1] < rtrace


def test_midsize_properties(env):
    """N = 100 000 (391 workgroups, the last one partial), D = 8, m = 256: more than one chunk of pivot coefficients."""
    c = dict(kind="sqexponential", scale=1.5, variance=1.3)
    N, D, m = 100_000, 8, 256
    X = np.random.default_rng(5).random((N, D))
    got = _run(env, c, X, m)
    assert got["selected"] == m
    idx = got["indices"]
    assert idx[0] == 0 and len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(got["trace"]) <= 0.0)
    resid = c["variance"] - np.sum(got["factor"] ** 2, axis=1)
    rel = abs(np.sum(resid) - got["trace"][-1]) / got["trace"][-1]
    print(f"midsize: trace {got['trace'][-1]:.6e}, recomputed from the factor {np.sum(resid):.6e}, rel {rel:.2e}")
    assert rel <= 1e-9
    assert np.array_equal(_bits(got["Z"]), _bits(X[idx]))
