"""QuadratureVI on the MI355X (VGP and SVGP on AGP_FLAG_NUMERICAL handles) against the NumPy restatement tests/_nvi_ref.py.
The inputs are tests/_nvi_cases.py; tests/test_nvi_host.py asserts the margin condition on every one of them, under which the alpha
histories of host and device must agree exactly.
"""
import ctypes as C

import numpy as np
import pytest

import _nvi_cases as CS
import _nvi_ref as Q
from _liks import agp_lik, oracle_lik
from _pitched import Pitched, layouts

pytestmark = pytest.mark.gpu

KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel"}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    return dict(AGP=AGP, capi=capi, R=R, torch=torch)


def _opt(AGP, name):
    return {"descent": lambda: AGP.Descent(0.1), "momentum": lambda: AGP.Momentum(1e-5), "adam": lambda: AGP.ADAM(0.01)}[name]()


def _model(AGP, case, n=100):
    X, y, mean = CS.data(case)
    tr = AGP.ScaleTransform(case["scale"]) if np.isscalar(case["scale"]) else AGP.ARDTransform(list(case["scale"]))
    k = 1.5 * (getattr(AGP, KERNELS[case["kind"]])() @ tr)
    inf = AGP.QuadratureVI(nGaussHermite=n, optimiser=_opt(AGP, case["opt"]), natural=case["natural"])
    return AGP.VGP(X, y, k, agp_lik(AGP, case["lik"]), inf, optimiser=False, mean=mean)


# ---- the quadrature kernel point by point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("likname", CS.LIKS)
@pytest.mark.parametrize("n", [3, 20, 100])
def test_quad_expectations_point_by_point(env, likname, n):
    """1000 points, var from 1e-12 to 1e2, |mu| up to 30: each of ell, g, h within 1e-12 of sum_j w_j |term_j| (the bound
    tests/test_gpu_mcgp.py puts on device transcendentals per point)"""
    AGP, R = env["AGP"], env["R"]
    rng = np.random.default_rng(n)
    P = 1000
    mu = rng.uniform(-30, 30, P)
    var = 10.0 ** rng.uniform(-12, 2, P)
    var[:3] = (1e-12, 1e2, 0.0)
    lik = oracle_lik(R, likname)
    y = np.sign(rng.standard_normal(P)) if likname == "logistic" else mu + 2.0 * rng.standard_normal(P)
    x, w = Q.gh_rule(n)
    ell, g, h = AGP.quad_expectations(agp_lik(AGP, likname), y, mu, var, x, w)
    er, gr, hr, (ea, ga, ha) = Q.expectations(lik, y, mu, var, x, w)
    tiny = np.finfo(np.float64).tiny
    errs = [float(np.max(np.abs(a - b) / np.maximum(s, tiny))) for a, b, s in ((ell, er, ea), (g, gr, ga), (h, hr, ha))]
    print(f"{likname} n={n}: worst errors relative to sum w |term|: ell {errs[0]:.2e} g {errs[1]:.2e} h {errs[2]:.2e}")
    assert np.all(np.isfinite(ell)) and np.all(np.isfinite(g)) and np.all(np.isfinite(h))
    assert max(errs) < 1e-12


# ---- VGP parity along a trajectory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.VGP_CASES))
def test_vgp_trajectory_parity(env, name):
    """20 steps (7 cells: the 8 or 10 for which the restated chain is a reference, tests/_nvi_cases.py): mu and Sigma within 1e-8
    (relative, max norm) and the ELBO within rtol 1e-8 after every step; the alpha history, the halving count and the rejected
    count equal"""
    AGP = env["AGP"]
    from agp_amd import nvi

    tr = CS.trajectory(name)
    model = _model(AGP, CS.VGP_CASES[name])
    emu, esig, eel = [], [], []
    for it in range(CS.steps_of(name)):
        AGP.train_(model, 1, state=None if it == 0 else True)
        mu, Sig = model.get_state(0)
        emu.append(_rel(mu, tr["mu"][it]))
        esig.append(_rel(Sig, tr["Sigma"][it]))
        eel.append(abs(AGP.objective(model) - tr["elbo"][it]) / max(1.0, abs(tr["elbo"][it])))
    a_last, halvings, rejected = nvi.nvi_info(model)
    print(f"{name}: mu {max(emu):.2e} Sigma {max(esig):.2e} ELBO {max(eel):.2e}; halvings {halvings}; alphas {model.nvi_alphas}")
    print("  per step mu    " + " ".join(f"{e:.1e}" for e in emu))
    print("  per step Sigma " + " ".join(f"{e:.1e}" for e in esig))
    assert model.nvi_alphas == tr["alphas"]
    assert (halvings, rejected) == (tr["halvings"], tr["rejected"]) and a_last == tr["alphas"][-1]
    assert max(emu) < 1e-8 and max(esig) < 1e-8 and max(eel) < 1e-8


def _sparse_model(AGP, case):
    X, y, Z, idx = CS.sparse_data(case)
    k = 1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0))
    kw = dict(nGaussHermite=100, optimiser=_opt(AGP, case["opt"]), natural=case["natural"])
    inf = AGP.QuadratureSVI(CS.SPARSE["B"], **kw) if case["stoch"] else AGP.QuadratureVI(**kw)
    return X, y, idx, AGP.SVGP(k, agp_lik(AGP, case["lik"]), inf, Z, optimiser=False)


@pytest.mark.parametrize("name", list(CS.SPARSE_CASES))
def test_svgp_trajectory_parity(env, name):
    """m = 70, N = 400, D = 3, 15 steps, QuadratureVI (B = N) and QuadratureSVI(150) on the restatement's index stream: mu, Sigma
    (1e-8 relative, max norm) and the ELBO on the step's batch (rtol 1e-8) after every step; alpha history and counters equal"""
    AGP = env["AGP"]
    from agp_amd import nvi

    case = CS.SPARSE_CASES[name]
    tr = CS.sparse_trajectory(name)
    X, y, idx, model = _sparse_model(AGP, case)
    emu, esig, eel = [], [], []
    for it in range(CS.SPARSE["steps"]):
        AGP.train_(model, X, y, 1, state=None if it == 0 else True, idx_stream=None if idx is None else [idx[it]])
        mu, Sig = model.get_state(0)
        emu.append(_rel(mu, tr["mu"][it]))
        esig.append(_rel(Sig, tr["Sigma"][it]))
        eel.append(abs(AGP.objective(model) - tr["elbo"][it]) / max(1.0, abs(tr["elbo"][it])))
    a_last, halvings, rejected = nvi.nvi_info(model)
    print(f"{name}: mu {max(emu):.2e} Sigma {max(esig):.2e} ELBO {max(eel):.2e}; halvings {halvings}; alphas {model.nvi_alphas}")
    print("  per step mu    " + " ".join(f"{e:.1e}" for e in emu))
    print("  per step Sigma " + " ".join(f"{e:.1e}" for e in esig))
    assert model.nvi_alphas == tr["alphas"]
    assert (halvings, rejected) == (tr["halvings"], tr["rejected"])
    assert max(emu) < 1e-8 and max(esig) < 1e-8 and max(eel) < 1e-8
    if name in ("logistic-svi-nat-descent", "studentt-vi-cla-adam"):  # predictions of the sparse posterior
        Xt = np.random.default_rng(1).standard_normal((57, 3))
        mr, vr = tr["ref"].predict_f(Xt)
        mf, vf = AGP.predict_f(model, Xt, cov=True)
        assert _rel(mf, mr) < 1e-8 and _rel(vf, vr) < 1e-6


def test_svgp_save_load_and_a_larger_batch(env, tmp_path):
    """QuadratureSVI: 5 steps, save, load, 4 more equal 9 uninterrupted bitwise; an ELBO on more points than the batch re-creates the
    handle and carries (mu, Sigma) and the optimiser state"""
    AGP = env["AGP"]
    from agp_amd import nvi

    case = CS.SPARSE_CASES["studentt-svi-cla-adam"]
    X, y, idx, a = _sparse_model(AGP, case)
    AGP.train_(a, X, y, 9, idx_stream=idx[:9])
    _, _, _, b = _sparse_model(AGP, case)
    AGP.train_(b, X, y, 5, idx_stream=idx[:5])
    AGP.save_trained_model(str(tmp_path / "s"), b)
    c = AGP.load_trained_model(str(tmp_path / "s"))
    assert repr(c.inference) == repr(a.inference) and c.inference.batchsize == CS.SPARSE["B"]
    AGP.train_(c, X, y, 4, state=True, idx_stream=idx[5:9])
    for u, v in zip(a.get_state(0) + nvi.get_opt_state(a)[:2], c.get_state(0) + nvi.get_opt_state(c)[:2]):
        assert np.array_equal(u, v)
    before = a.get_state(0) + nvi.get_opt_state(a)
    a._ensure_handle(len(X))  # (what an evaluation on the whole set asks for)
    after = a.get_state(0) + nvi.get_opt_state(a)
    assert all(np.array_equal(u, v) for u, v in zip(before, after))


def test_fixed_point_on_the_device(env):
    """Logistic, natural, Descent(0.1), n = 100, N = 40, 300 steps: the Opper-Archambeau residuals mu - K g and
    Sigma^-1 - (K^-1 - Diagonal(h)), computed in NumPy from the device's mu and Sigma, below 1e-8"""
    AGP = env["AGP"]
    X, y = CS.fixed_point_problem()
    ref, _ = CS.fixed_point_reference()
    inf = AGP.QuadratureVI(nGaussHermite=100, optimiser=AGP.Descent(0.1))
    model = AGP.VGP(X, y, 2.0 * AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), inf, optimiser=False)
    AGP.train_(model, CS.FIXED_POINT["steps"])
    mu, Sig = model.get_state(0)
    _, g, h, _ = Q.expectations(ref.lik, y, mu, np.diag(Sig), ref.x, ref.w)
    r1, r2 = Q.fixed_point_residuals(ref.K, ref.mu0, mu, Sig, g, h)
    print(f"residuals {r1:.2e} {r2:.2e}; smallest alpha {min(model.nvi_alphas)}")
    assert model.nvi_alphas == ref.alphas
    assert r1 < 1e-8 and r2 < 1e-8


@pytest.mark.parametrize("name", ["logistic-130-nat-descent", "studentt-63-nat-descent-empmean", "laplace-130-nat-descent-ardmatern52"])
def test_predictions_after_training(env, name):
    """predict_f, proba_y and predict_y against the restatement at the bounds tests/test_gpu_vgp.py uses (1e-8 on means, 1e-6 on
    variances: k** - diag(K*n A Kn*) cancels digits of A)"""
    AGP, R = env["AGP"], env["R"]
    tr = CS.trajectory(name)
    ref = tr["ref"]
    model = _model(AGP, CS.VGP_CASES[name])
    AGP.train_(model, CS.steps_of(name))
    Xt = np.random.default_rng(1).standard_normal((57, 3))
    mr, vr = ref.predict_f(Xt)
    mf, vf = AGP.predict_f(model, Xt, cov=True)
    assert _rel(mf, mr) < 1e-8 and _rel(vf, vr) < 1e-6
    assert _rel(AGP.predict_f(model, Xt), mr) < 1e-8
    pa = AGP.proba_y(model, Xt)
    pr = R.compute_proba(ref.lik, (mr,), (vr,))
    assert _rel(pa[0], pr[0]) < 1e-8 and _rel(pa[1], pr[1]) < 1e-6
    # the ELBO's other doors: the enqueued form (evaluated synchronously on this handle) and ELBO(model) (no local variables to refresh)
    e = AGP.objective(model)
    assert AGP.objective_fetch(model, AGP.objective_enqueue(model)) == e and AGP.ELBO(model) == e
    assert abs(e - tr["elbo"][-1]) < 1e-8 * max(1.0, abs(tr["elbo"][-1]))
    py = AGP.predict_y(model, Xt)
    if ref.lik.name == "logistic":
        assert np.array_equal(np.asarray(py), mr > 0)
    else:
        assert _rel(py, mr) < 1e-8


@pytest.mark.parametrize("name", ["logistic-63-nat-momentum", "studentt-63-cla-adam", "laplace-130-nat-descent"])
def test_save_load_continues_bit_for_bit(env, name, tmp_path):
    """7 steps, save, load, 6 more with state= : mu, Sigma, the moments and the ELBO equal those of 13 uninterrupted steps bitwise"""
    AGP = env["AGP"]
    from agp_amd import nvi

    case = CS.VGP_CASES[name]
    a = _model(AGP, case)
    AGP.train_(a, 13)
    b = _model(AGP, case)
    AGP.train_(b, 7)
    AGP.save_trained_model(str(tmp_path / "m"), b)
    c = AGP.load_trained_model(str(tmp_path / "m"))
    assert repr(c.inference) == repr(a.inference) and c.inference.n_iter == 7
    assert c.inference.natural == case["natural"] and type(c.inference.nvi_optimiser) is type(a.inference.nvi_optimiser)
    AGP.train_(c, 6, state=True)
    for u, v in zip(a.get_state(0) + nvi.get_opt_state(a)[:2], c.get_state(0) + nvi.get_opt_state(c)[:2]):
        assert np.array_equal(u, v)
    assert nvi.get_opt_state(a)[2] == nvi.get_opt_state(c)[2] == 13
    assert AGP.objective(a) == AGP.objective(c)
    assert a.nvi_alphas[7:] == c.nvi_alphas


# ---- the ABI: layout contract and refusals ----------------------------------------------------------------------------------------
def _handle(env, flags, lik=None, dtype=None, N=20, D=2, stochastic=0):
    capi, torch = env["capi"], env["torch"]
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    d = capi.SvgpDesc()
    d.dtype = capi.F64 if dtype is None else dtype
    d.n_latent, d.latent_offset, d.stochastic = 1, 0, stochastic
    d.m, d.D, d.max_batch = N, D, N
    d.lik = lik if lik is not None else capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0)
    d.rm_kappa, d.rm_tau = 0.51, 1.0
    d.flags = flags
    h = C.c_void_p()
    st = L.agp_svgp_create(ctx, C.byref(d), C.byref(h))
    return L, ctx, h, st


def test_step_never_touches_x(env):
    """agp_svgp_nvi_step takes (x, ldx) like the CAVI step but reads the handle's own inputs: the same bits with x = NULL, a
    contiguous x and NaN-guarded pitched x in every layout; the guards stay intact"""
    AGP, torch = env["AGP"], env["torch"]
    case = CS.VGP_CASES["logistic-63-nat-descent"]
    X = CS.data(case)[0]
    results = []
    variants = [None, ("contiguous",)] + layouts(X.shape[1], "f64")
    for v in variants:
        model = _model(AGP, case)
        h = model._ensure_handle()
        yd = model._upload_y(model._treat(model.y))
        L = env["capi"].lib()
        if v is None:
            ptr, ld, p = None, 0, None
        elif v == ("contiguous",):
            xt = torch.as_tensor(X, device="cuda").contiguous()
            ptr, ld, p = C.c_void_p(xt.data_ptr()), X.shape[1], None
        else:
            p = Pitched("f64", data=X, ld=v[0], off=v[1], device="cuda")
            ptr, ld = C.c_void_p(p.ptr), p.ld
        for _ in range(3):
            model._chk(L.agp_svgp_nvi_step(h, ptr, ld, C.c_void_p(yd.data_ptr()), None, len(X), 1.0))
        if p is not None:
            p.check("x of agp_svgp_nvi_step")
        results.append(model.get_state(0))
    for mu, Sig in results[1:]:
        assert np.array_equal(mu, results[0][0]) and np.array_equal(Sig, results[0][1])
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(Sig))


def test_sparse_step_with_pitched_x(env):
    """the sparse step reads (x, ldx): contiguous and NaN-guarded pitched x in every layout give the same bits, guards intact;
    ldx = D - 1 is refused without touching the state"""
    AGP, torch = env["AGP"], env["torch"]
    case = CS.SPARSE_CASES["logistic-svi-nat-descent"]
    results = []
    for v in [None] + layouts(CS.SPARSE["D"], "f64"):
        X, y, idx, model = _sparse_model(AGP, case)
        AGP.train_(model, X, y, 1, idx_stream=idx[:1])  # (creates the handle, uploads y)
        h, (Xd, yd, N) = model._h, model._data
        L = env["capi"].lib()
        it = torch.as_tensor(idx[1], device="cuda")
        p = None if v is None else Pitched("f64", data=X, ld=v[0], off=v[1], device="cuda")
        ptr, ld = (C.c_void_p(Xd.data_ptr()), Xd.stride(0)) if p is None else (C.c_void_p(p.ptr), p.ld)
        rho = N / CS.SPARSE["B"]
        assert L.agp_svgp_nvi_step(h, ptr, CS.SPARSE["D"] - 1, C.c_void_p(yd.data_ptr()), C.c_void_p(it.data_ptr()), len(idx[1]), rho) == 1
        model._chk(L.agp_svgp_nvi_step(h, ptr, ld, C.c_void_p(yd.data_ptr()), C.c_void_p(it.data_ptr()), len(idx[1]), rho))
        out = C.c_double()
        model._chk(L.agp_svgp_elbo(h, ptr, ld, C.c_void_p(yd.data_ptr()), C.c_void_p(it.data_ptr()), len(idx[1]), rho, 0, C.byref(out)))
        if p is not None:
            p.check("x of agp_svgp_nvi_step / agp_svgp_elbo")
        results.append(model.get_state(0) + (np.array(out.value),))
    for r in results[1:]:
        assert all(np.array_equal(u, v) and np.all(np.isfinite(u)) for u, v in zip(r, results[0]))


def test_refusals_through_the_abi(env):
    capi, torch = env["capi"], env["torch"]
    FULL, NUM = capi.FLAG_FULL, capi.FLAG_NUMERICAL
    INV, NOT_POSDEF, BAD_BATCH, UNS = 1, 2, 4, 5  # AGP_ERR_INVALID, _NOT_POSDEF, _BAD_BATCH, _UNSUPPORTED (include/agp_hip.h)

    def refused(flags, want, **kw):
        L, ctx, h, st = _handle(env, flags, **kw)
        assert st == want, (flags, kw, st)
        msg = L.agp_last_error(ctx).decode()
        L.agp_ctx_destroy(ctx)
        return msg

    assert "not compatible" in refused(NUM, UNS, lik=capi.LikDesc(capi.LIK_GAUSSIAN, 1, 0.1, 0.0))   # the sparse handle
    refused(NUM, UNS, dtype=capi.F32)
    assert "Logistic, StudentT and Laplace" in refused(NUM, UNS, lik=capi.LikDesc(capi.LIK_POISSON, 1, 2.0, 0.0))
    assert "AGP_FLAG_NUMERICAL" in refused(NUM | FULL | capi.FLAG_SAMPLED, UNS)
    assert "AGP_FLAG_NUMERICAL" in refused(NUM | FULL | capi.FLAG_EXACT, UNS)
    refused(NUM | FULL, UNS, dtype=capi.F32)
    assert "not compatible" in refused(NUM | FULL, UNS, lik=capi.LikDesc(capi.LIK_GAUSSIAN, 1, 0.1, 0.0))
    for kind in (capi.LIK_BAYESIANSVM, capi.LIK_POISSON, capi.LIK_NEGBINOMIAL):
        assert "Logistic, StudentT and Laplace" in refused(NUM | FULL, UNS, lik=capi.LikDesc(kind, 1, 2.0, 0.0))
    refused(NUM | FULL, INV, stochastic=1)

    N, D = 20, 2
    rng = np.random.default_rng(0)
    Xd = torch.as_tensor(rng.standard_normal((N, D)), device="cuda")
    yd = torch.as_tensor(np.sign(rng.standard_normal(N)), device="cuda")
    idx = torch.arange(N, device="cuda")
    x, w = Q.gh_rule(20)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda t: C.c_void_p(t.data_ptr())

    L, ctx, h, st = _handle(env, NUM | FULL, N=N, D=D)
    assert st == 0
    assert L.agp_svgp_set_Z(h, 0, vp(Xd), D) == 0
    step = lambda B=N, ix=None, rho=1.0: L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), ix, B, rho)
    assert step() == INV and "agp_svgp_nvi_configure" in L.agp_last_error(ctx).decode()   # no rule installed yet
    assert L.agp_svgp_nvi_configure(h, 0, dp(x), dp(w), 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == INV
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, 7, 0.1, 0.0, 0.0, 0.0) == INV
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, capi.OPT_MOMENTUM, 0.1, 1.5, 0.0, 0.0) == INV
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == 0
    assert step(B=N - 1) == BAD_BATCH and step(ix=vp(idx)) == BAD_BATCH
    assert step(rho=2.0) == INV
    assert L.agp_svgp_cavi_step(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert "agp_svgp_nvi_step" in L.agp_last_error(ctx).decode()
    assert L.agp_svgp_hyper_step(h) == UNS
    dv, ds = C.c_double(), (C.c_double * D)()
    assert L.agp_svgp_hypergrad(h, 0, C.byref(dv), ds, None) == UNS
    assert L.agp_svgp_step_local(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert step() == 0
    mu, e1 = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    assert L.agp_svgp_get_state(h, 0, vp(mu), None, vp(e1), None) == UNS
    bad = torch.eye(N, dtype=torch.float64, device="cuda")
    bad[3, 3] = -1.0
    assert L.agp_svgp_set_state(h, 0, vp(mu), vp(bad)) == NOT_POSDEF
    a, hv, rj = C.c_double(), C.c_int64(), C.c_int64()
    assert L.agp_svgp_nvi_info(h, 1, C.byref(a), C.byref(hv), C.byref(rj)) == INV
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx)

    L, ctx, h, st = _handle(env, FULL, N=N, D=D)   # an AnalyticVI handle refuses the numerical entry points
    assert st == 0
    assert L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == UNS
    assert L.agp_svgp_nvi_info(h, 0, C.byref(a), C.byref(hv), C.byref(rj)) == UNS
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx)

    ell = torch.empty(N, dtype=torch.float64, device="cuda")
    L, ctx, h, st = _handle(env, FULL, N=N, D=D)
    lg = capi.LikDesc(capi.LIK_POISSON, 1, 2.0, 0.0)
    assert L.agp_quad_expectations(ctx, C.byref(lg), vp(yd), vp(mu), vp(mu), N, dp(x), dp(w), 20, vp(ell), vp(ell), vp(ell)) == UNS
    ls = capi.LikDesc(capi.LIK_STUDENTT, 1, 3.0, 0.0)  # sigma = 0
    assert L.agp_quad_expectations(ctx, C.byref(ls), vp(yd), vp(mu), vp(mu), N, dp(x), dp(w), 20, vp(ell), vp(ell), vp(ell)) == INV
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx)


def test_sparse_handle_refusals(env):
    capi, torch = env["capi"], env["torch"]
    INV, BAD_BATCH, UNS = 1, 4, 5
    N, D, m = 40, 2, 20
    rng = np.random.default_rng(0)
    Xd = torch.as_tensor(rng.standard_normal((N, D)), device="cuda")
    yd = torch.as_tensor(np.sign(rng.standard_normal(N)), device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    L, ctx, h, st = _handle(env, capi.FLAG_NUMERICAL, N=m, D=D, stochastic=1)
    assert st == 0
    L.agp_svgp_destroy(h)
    d = capi.SvgpDesc()
    d.dtype, d.n_latent, d.m, d.D, d.max_batch = capi.F64, 1, m, D, N
    d.lik, d.rm_kappa, d.rm_tau, d.flags = capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0), 0.51, 1.0, capi.FLAG_NUMERICAL
    h = C.c_void_p()
    assert L.agp_svgp_create(ctx, C.byref(d), C.byref(h)) == 0
    assert L.agp_svgp_set_Z(h, 0, vp(Xd), D) == 0
    x, w = Q.gh_rule(20)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == 0
    assert L.agp_svgp_nvi_step(h, None, D, vp(yd), None, N, 1.0) == INV           # the sparse step reads x
    assert L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), None, N + 1, 1.0) == BAD_BATCH
    assert L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), None, N, 0.0) == INV
    assert L.agp_svgp_cavi_step(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert L.agp_svgp_step_local(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert L.agp_svgp_prefetch(h, vp(Xd), D, None, N) == UNS
    assert L.agp_svgp_hyper_step(h) == UNS
    assert L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), None, N, 1.0) == 0
    assert L.agp_svgp_check_status(h) == 0
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx)
