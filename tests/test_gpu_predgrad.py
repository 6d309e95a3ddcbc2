"""agp_svgp_predict_f_grad / predict_f_grad on the MI355X: the input gradients of the predictive mean and variance against the NumPy
restatement tests/_predgrad_ref.py fed with the oracle models of tests/_predgrad_cases.py (whose conditioning the CPU suite
asserts), test points on inducing points, cov=False, determinism, side effects, the layout contract, fp32 and the refusals.

PARITY is the project's parity bound: relative 1e-8 in max norm per output array.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _predgrad_cases as PC
import _predgrad_ref as G
from _pitched import Pitched

pytestmark = pytest.mark.gpu

PARITY = 1e-8
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, L=capi.lib(), torch=torch)


@functools.lru_cache(maxsize=None)
def _model(name):
    """the trained device model of a case, shared by the tests (none of them changes it: that is one of the tests)"""
    import agp_amd as AGP

    return PC.make_model(AGP, name)


def _svgp(model):
    return model._cur if hasattr(model, "_cur") else model


def _raw(L, model, xt_ptr, ldx, nt, dmu_ptr, dvar_ptr, ldg):
    """the C entry point itself -> status"""
    m = _svgp(model)
    h = m._ensure_handle(max(m._max_batch, 1))
    st = L.agp_svgp_predict_f_grad(h, C.c_void_p(xt_ptr) if xt_ptr else None, ldx, nt, C.c_void_p(dmu_ptr) if dmu_ptr else None,
                                   C.c_void_p(dvar_ptr) if dvar_ptr else None, ldg)
    L.agp_ctx_sync(m._ctx)
    return st


def _outputs(res, cov=True):
    """predict_f_grad's return value -> (list of dmu arrays, list of dvar arrays)"""
    gm, gv = res if cov else (res, None)
    if isinstance(gm, tuple):
        return list(gm), (list(gv) if cov else None)
    return [gm], ([gv] if cov else None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- (a) parity, fp64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_parity_fp64(env, name):
    AGP = env["AGP"]
    ref = PC.reference(name)
    wm, wv = PC.restated(name)
    gm, gv = _outputs(AGP.predict_f_grad(_model(name), ref["Xt"]))
    assert len(gm) == len(wm) and len(gv) == len(wv)
    errs = []
    for k in range(len(wm)):
        assert gm[k].shape == wm[k].shape == gv[k].shape and gm[k].dtype == np.float64
        assert np.all(np.isfinite(gm[k])) and np.all(np.isfinite(gv[k]))
        errs.append((G.rel(gm[k], wm[k]), G.rel(gv[k], wv[k])))
    print(f"{name}: " + "  ".join(f"[{k}] dmu {a:.2e} dvar {b:.2e}" for k, (a, b) in enumerate(errs)))
    assert max(max(e) for e in errs) <= PARITY


# ---- (b) test points on inducing points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["svgp-logistic-m65-m32-ard", "svgp-logistic-d1-m63-m52-ard"])
def test_points_on_inducing_points(env, name):
    """X_test = Z plus one random point: a coinciding pair is an ordinary input (Matern32 and Matern52: phi' is finite at r = 0 and
    nothing divides by r)"""
    AGP = env["AGP"]
    assert PC.CASES[name]["kind"] in ("matern32", "matern52")
    d = PC.data(name)
    Xt = np.vstack([d["Z"], d["Xt"][:1]])
    wm, wv = PC.restated(name, Xt=Xt)
    gm, gv = AGP.predict_f_grad(_model(name), Xt)
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    em, ev = G.rel(gm, wm[0]), G.rel(gv, wv[0])
    print(f"{name}: on the inducing points  dmu {em:.2e}  dvar {ev:.2e}")
    assert em <= PARITY and ev <= PARITY


# ---- (c) cov=False ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["svgp-gaussian-m130-nt4133-sq-scale", "svgp-softmax3-m65-sq-scale", "mosvgp-2tasks-3latents-m63"])
def test_cov_false(env, name):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    model, Xt = _model(name), PC.reference(name)["Xt"]
    gm, _ = _outputs(AGP.predict_f_grad(model, Xt))
    only, none = _outputs(AGP.predict_f_grad(model, Xt, cov=False), cov=False)
    assert none is None and len(only) == len(gm)
    for a, b in zip(only, gm):
        assert np.array_equal(_bits(a), _bits(b))
    # through the ABI: dvar_out = NULL writes dmu_out alone, the same bits
    Xd = model._upload(Xt)
    nt, D = Xd.shape
    out = torch.full((len(gm), nt, D), float("nan"), dtype=torch.float64, device="cuda")
    assert _raw(L, model, Xd.data_ptr(), D, nt, out.data_ptr(), 0, D) == 0
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(np.stack(gm)))


# ---- (d) determinism ----------------------------------------------------------------------------------------------------------------------
def test_determinism(env):
    AGP = env["AGP"]
    name = "svgp-gaussian-m130-nt4133-sq-scale"
    model, Xt = _model(name), PC.reference(name)["Xt"]
    assert len(Xt) == 4096 + 37
    a = AGP.predict_f_grad(model, Xt)
    b = AGP.predict_f_grad(model, Xt)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    # a point's result does not depend on where it stands in the stream, up to the products in front of the kernel
    c = AGP.predict_f_grad(model, Xt[:100])
    em = float(np.max(np.abs(a[0][:100] - c[0])) / np.max(np.abs(c[0])))
    ev = float(np.max(np.abs(a[1][:100] - c[1])) / np.max(np.abs(c[1])))
    print(f"first 100 rows of n_t = 4133 against n_t = 100: dmu {em:.2e} dvar {ev:.2e}")
    assert em <= PARITY and ev <= PARITY


# ---- (e) no side effects --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["svgp-logistic-m65-m32-ard", "svgp-softmax3-m65-sq-scale"])
def test_no_side_effects(env, name):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    model, Xt = PC.make_model(AGP, name), PC.reference(name)["Xt"]  # a model of its own: fresh caches

    def snapshot():
        terms = (C.c_double * 3)()
        model._chk(L.agp_svgp_elbo_terms(model._h, terms))
        snap = [np.asarray(tuple(terms))]
        for l in range(model.n_latent):
            snap += list(model.get_state(l))
            snap += [model.get_matrix(w, l) for w in (capi.VEC_THETA, capi.VEC_C, capi.VEC_MEAN_F)]
        return snap

    e0 = AGP.objective(model)
    before = snapshot()
    p0 = _outputs(AGP.predict_f(model, Xt, cov=True))
    AGP.predict_f_grad(model, Xt)
    AGP.predict_f_grad(model, Xt, cov=False)
    assert L.agp_svgp_check_status(model._h) == 0
    after = snapshot()
    p1 = _outputs(AGP.predict_f(model, Xt, cov=True))
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    for a, b in zip(p0[0] + p0[1], p1[0] + p1[1]):
        assert np.array_equal(_bits(a), _bits(b))
    assert AGP.objective(model) == e0
    # ... and a call BEFORE the first prediction leaves the same predictions behind as none
    fresh = PC.make_model(AGP, name)
    AGP.predict_f_grad(fresh, Xt)
    p2 = _outputs(AGP.predict_f(fresh, Xt, cov=True))
    for a, b in zip(p0[0] + p0[1], p2[0] + p2[1]):
        assert np.array_equal(_bits(a), _bits(b))


# ---- (f) layout -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["svgp-logistic-m65-m32-ard", "svgp-softmax3-m65-sq-scale", "svgp-gaussian-d64-m64-sq-ard",
                                  "mosvgp-2tasks-3latents-m63"])
def test_layout(env, name):
    """pitched xt (ldx = D + 3) and pitched outputs (ldg = D + 5) inside NaN guard bands: the same bits as the contiguous call, the
    bands untouched, every element of the windows written"""
    AGP, L = env["AGP"], env["L"]
    model, Xt = _model(name), PC.reference(name)["Xt"]
    nt, D = Xt.shape
    gm, gv = _outputs(AGP.predict_f_grad(model, Xt))
    nout = len(gm)
    xin = Pitched("f64", data=Xt, ld=D + 3, off=1, device="cuda")
    om = Pitched("f64", rows=nout * nt, width=D, ld=D + 5, off=1, device="cuda")
    ov = Pitched("f64", rows=nout * nt, width=D, ld=D + 5, off=0, device="cuda")
    assert _raw(L, model, xin.ptr, D + 3, nt, om.ptr, ov.ptr, D + 5) == 0
    xin.check("xt")
    om.check("dmu_out")
    ov.check("dvar_out")
    assert not om.unwritten().any() and not ov.unwritten().any()
    assert np.array_equal(_bits(om.window()), _bits(np.concatenate(gm)))
    assert np.array_equal(_bits(ov.window()), _bits(np.concatenate(gv)))
    # means only: dvar_out is not touched
    om2 = Pitched("f64", rows=nout * nt, width=D, ld=D + 5, off=0, device="cuda")
    assert _raw(L, model, xin.ptr, D + 3, nt, om2.ptr, 0, D + 5) == 0
    om2.check("dmu_out (means only)")
    assert np.array_equal(_bits(om2.window()), _bits(np.concatenate(gm)))


# ---- (g) fp32 -------------------------------------------------------------------------------------------------------------------------------
def test_fp32(env):
    """against the fp64 restatement (the oracle with the reference's Float32 jitter, 1e-3).  Bound: 4 x the error of the EXISTING fp32
    predict_f variance against the fp64 oracle on the same case -- the gradient adds a D-term scaling and one more product to the
    same accumulations."""
    AGP = env["AGP"]
    name = PC.FP32_CASE
    ref = PC.reference(name, 1e-3)
    Xt = ref["Xt"]
    model = PC.make_model(AGP, name, T=np.float32)
    mu, var = AGP.predict_f(model, Xt, cov=True)
    mu_r, var_r = G.moments(Xt, *ref["parts"][0], jitter=ref["jitter"])
    e_mu, e_var = G.rel(mu, mu_r), G.rel(var, var_r)
    wm, wv = PC.restated(name, jitter=1e-3)
    gm, gv = AGP.predict_f_grad(model, Xt)
    assert gm.dtype == np.float32 and gv.dtype == np.float32
    em, ev = G.rel(gm, wm[0]), G.rel(gv, wv[0])
    print(f"fp32 {name}: predict_f mean {e_mu:.3e} variance {e_var:.3e} (bound 4 x variance = {4 * e_var:.3e}); "
          f"predict_f_grad dmu {em:.3e} dvar {ev:.3e}")
    assert em <= 4 * e_var and ev <= 4 * e_var


# ---- (h) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    rng = np.random.default_rng(0)

    def sparse(kernel, D):
        X = rng.standard_normal((40, D))
        y = np.where(X[:, 0] > 0, 1, -1)
        m = AGP.SVGP(kernel, AGP.LogisticLikelihood(), AGP.AnalyticSVI(20), X[:6].copy(), optimiser=False)
        AGP.train_(m, X, y, 2)
        return m, X

    X2 = rng.standard_normal((40, 2))
    mc = AGP.MCGP(X2, np.where(X2[:, 0] > 0, 1, -1), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    cases = [("ExponentialKernel", UNSUPPORTED, 0) + sparse(AGP.ExponentialKernel(), 3),
             ("at most 64", UNSUPPORTED, 0) + sparse(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.2), 65),
             ("AGP_FLAG_SAMPLED", UNSUPPORTED, 0, mc, X2),
             ("ldg >= D", INVALID, -1) + sparse(AGP.Matern32Kernel(), 3)]
    for what, status, dld, model, X in cases:
        nt, D = X.shape
        Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
        ldg = D + dld
        om = torch.full((nt * D,), float("nan"), dtype=torch.float64, device="cuda")
        ov = torch.full((nt * D,), float("nan"), dtype=torch.float64, device="cuda")
        st = _raw(L, model, Xd.data_ptr(), D, nt, om.data_ptr(), ov.data_ptr(), ldg)
        msg = L.agp_last_error(model._ctx).decode()
        assert st == status, (what, st, msg)
        assert "agp_svgp_predict_f_grad" in msg and what in msg, (what, msg)
        assert bool(torch.isnan(om).all()) and bool(torch.isnan(ov).all()), what  # untouched
        if model is not mc:  # the handle still predicts
            mu, var = AGP.predict_f(model, X, cov=True)
            assert np.all(np.isfinite(mu)) and np.all(var > 0)
    # the other argument checks, and n_t = 0
    model, X = cases[3][3], cases[3][4]
    Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
    om = torch.full((40 * 3,), float("nan"), dtype=torch.float64, device="cuda")
    assert _raw(L, model, Xd.data_ptr(), 2, 40, om.data_ptr(), 0, 3) == INVALID   # ldx < D
    assert _raw(L, model, Xd.data_ptr(), 3, -1, om.data_ptr(), 0, 3) == INVALID   # n_t < 0
    assert _raw(L, model, 0, 3, 40, om.data_ptr(), 0, 3) == INVALID                # xt NULL
    assert _raw(L, model, Xd.data_ptr(), 3, 40, 0, 0, 3) == INVALID                # dmu_out NULL
    assert _raw(L, model, Xd.data_ptr(), 3, 0, om.data_ptr(), 0, 3) == 0           # n_t = 0: a successful no-op
    assert bool(torch.isnan(om).all())
    assert _raw(L, model, Xd.data_ptr(), 3, 40, om.data_ptr(), 0, 3) == 0
    assert not bool(torch.isnan(om).any())
    # the host mirror decides the same refusals before the device is touched
    with pytest.raises(NotImplementedError, match="MCGP"):
        AGP.predict_f_grad(mc, X2)
    with pytest.raises(NotImplementedError, match="ExponentialKernel"):
        AGP.predict_f_grad(cases[0][3], cases[0][4])
