"""MCIntegrationVI on the MI355X (VGP and SVGP on AGP_FLAG_NUMERICAL | AGP_FLAG_MC handles) against the NumPy restatement
tests/_mcvi_ref.py.  The inputs are tests/_mcvi_cases.py; tests/test_mcvi_host.py asserts the margin condition on every one of them,
under which the alpha histories of host and device must agree exactly.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _mcvi_cases as CS
import _mcvi_ref as M
import _nvi_cases as QCS
from _liks import agp_lik
from _pitched import Pitched, layouts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nvi", "studentt_63_cla_adam_5steps.npz")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, torch=torch)


def _lik(AGP, link, K):
    return AGP.SoftMaxLikelihood(K) if link == "softmax" else AGP.LogisticSoftMaxLikelihood(K)


def _opt(AGP, name):
    return {"descent": lambda: AGP.Descent(0.1), "adam": lambda: AGP.ADAM(0.01)}[name]()


def _kernel(AGP):
    return CS.KVAR * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(CS.SCALE))


def _model(AGP, case, seed=CS.SEED):
    X, c = CS.data(case)
    inf = AGP.MCIntegrationVI(nMC=CS.NMC, optimiser=_opt(AGP, case["opt"]), natural=case["natural"], seed=seed)
    return AGP.VGP(X, c + 1, _kernel(AGP), _lik(AGP, case["link"], case["K"]), inf, optimiser=False)


def _sparse_model(AGP, case, seed=CS.SEED):
    X, c, Z, idx = CS.sparse_data(case)
    kw = dict(nMC=CS.NMC, optimiser=_opt(AGP, case["opt"]), natural=case["natural"], seed=seed)
    inf = AGP.MCIntegrationSVI(CS.SPARSE["B"], **kw) if case["stoch"] else AGP.MCIntegrationVI(**kw)
    return X, c + 1, idx, AGP.SVGP(_kernel(AGP), _lik(AGP, case["link"], CS.sparse_K(case)), inf, Z, optimiser=False)


def _full_state(model):
    from agp_amd import nvi

    out = []
    for k in range(model.n_latent):
        out += list(model.get_state(k)) + list(nvi.get_opt_state(model, latent=k)[:2])
    return out


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 8, 17, 64])
def test_mc_normals_bit_identical(env, K):
    """the device's table equals the host Philox table bit for bit: nMC in {1, 63, 200, 1000}, streams 2 and 3, two values of t"""
    AGP = env["AGP"]
    for nMC in (1, 63, 200, 1000):
        for stream in (M.STREAM_GRAD, M.STREAM_ELBO):
            for t in (1, 4000000000):
                d = AGP.mc_normals(CS.SEED, t, stream, nMC, K)
                h = M.normals(CS.SEED, t, stream, nMC, K)
                assert d.shape == (nMC, K) and np.array_equal(d, h), (nMC, stream, t, int(np.sum(d != h)))


# ---- 2. the expectation kernel point by point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", M.LINKS)
@pytest.mark.parametrize("K", [2, 3, 8])
def test_mc_expectations_point_by_point(env, link, K):
    """500 points, |mu| up to 30, var from 1e-12 to 1e2 and points at var = 0, nMC in {1, 63, 1000}: every ell, g, h finite and within
    1e-12 of (1 / nMC) sum_s |term_s| (the bound tests/test_gpu_nvi.py puts on the quadrature kernel) of the restatement fed the same
    table; two calls agree bitwise"""
    AGP = env["AGP"]
    c, mu, var = CS.point_inputs(K)
    lik = _lik(AGP, link, K)
    tiny = np.finfo(np.float64).tiny
    for nMC in (1, 63, 1000):
        ell, g, h = AGP.mc_expectations(lik, c, mu, var, nMC, CS.SEED, 5, M.STREAM_GRAD)
        er, gr, hr, (ea, ga, ha) = M.expectations(link, c, mu, var, M.normals(CS.SEED, 5, M.STREAM_GRAD, nMC, K))
        errs = [float(np.max(np.abs(a - b) / np.maximum(s, tiny))) for a, b, s in ((ell, er, ea), (g, gr, ga), (h, hr, ha))]
        print(f"{link} K={K} nMC={nMC}: worst errors relative to mean |term|: ell {errs[0]:.2e} g {errs[1]:.2e} h {errs[2]:.2e}")
        assert np.all(np.isfinite(ell)) and np.all(np.isfinite(g)) and np.all(np.isfinite(h))
        assert max(errs) < 1e-12
        again = AGP.mc_expectations(lik, c, mu, var, nMC, CS.SEED, 5, M.STREAM_GRAD)
        assert all(np.array_equal(a, b) for a, b in zip((ell, g, h), again))


# ---- 3., 4. parity along a trajectory ------------------------------------------------------------------------------------------------
def _assert_parity(AGP, model, tr, steps, train):
    from agp_amd import nvi

    K = model.n_latent
    emu, esig, eel = [], [], []
    for it in range(steps):
        train(it)
        for k in range(K):
            mu, Sig = model.get_state(k)
            emu.append(_rel(mu, tr["mu"][it][k]))
            esig.append(_rel(Sig, tr["Sigma"][it][k]))
        eel.append(abs(AGP.objective(model) - tr["elbo"][it]) / max(1.0, abs(tr["elbo"][it])))
    infos = [nvi.nvi_info(model, latent=k) for k in range(K)]
    print(f"mu {max(emu):.2e} Sigma {max(esig):.2e} ELBO {max(eel):.2e}; (halvings, rejected) {[i[1:] for i in infos]}")
    assert model.nvi_alphas == tr["alphas"]
    assert [i[1:] for i in infos] == tr["counters"] and tuple(i[0] for i in infos) == tr["alphas"][-1]
    assert max(emu) < 1e-8 and max(esig) < 1e-8 and max(eel) < 1e-8


@pytest.mark.parametrize("name", list(CS.VGP_CASES))
def test_vgp_trajectory_parity(env, name):
    """12 steps: mu_k and Sigma_k of every latent within 1e-8 (relative, max norm) and the ELBO within rtol 1e-8 after every step; the
    alpha tuples, the halving and the rejected counters equal (the tolerances of the QuadratureVI parity test)"""
    AGP = env["AGP"]
    model = _model(AGP, CS.VGP_CASES[name])
    _assert_parity(AGP, model, CS.trajectory(name), CS.VGP_STEPS, lambda it: AGP.train_(model, 1, state=None if it == 0 else True))


@pytest.mark.parametrize("name", list(CS.SPARSE_CASES))
def test_svgp_trajectory_parity(env, name):
    """m = 70, N = 400, D = 3, K = 3 (and one case at K = 10), 10 steps, MCIntegrationVI (B = N) and MCIntegrationSVI(150) on the restatement's index stream:
    the same assertions; then predict_f, predict_y and proba_y on 57 test points"""
    AGP = env["AGP"]
    case, tr = CS.SPARSE_CASES[name], CS.sparse_trajectory(name)
    X, y, idx, model = _sparse_model(AGP, case)
    _assert_parity(AGP, model, tr, CS.SPARSE["steps"],
                   lambda it: AGP.train_(model, X, y, 1, state=None if it == 0 else True, idx_stream=None if idx is None else [idx[it]]))
    Xt = np.random.default_rng(1).standard_normal((57, 3))
    mr, vr = tr["ref"].predict_f(Xt)
    mf, vf = AGP.predict_f(model, Xt, cov=True)
    assert _rel(np.stack(mf), mr) < 1e-8 and _rel(np.stack(vf), vr) < 1e-6
    assert _rel(np.stack(AGP.predict_f(model, Xt)), mr) < 1e-8
    pr = M.link_proba(case["link"], mr)
    pa = AGP.proba_y(model, Xt)
    labels = list(range(1, CS.sparse_K(case) + 1))
    assert sorted(pa) == labels and _rel(np.stack([pa[k] for k in labels], axis=1), pr) < 1e-8
    top2 = np.sort(mr, axis=0)
    clear = top2[-1] - top2[-2] > 1e-6
    assert clear.sum() > 40 and np.array_equal(np.asarray(AGP.predict_y(model, Xt))[clear], 1 + np.argmax(mr, axis=0)[clear])


# ---- 5. save / load, seeds -----------------------------------------------------------------------------------------------------------
def test_vgp_save_load_and_seeds(env, tmp_path):
    """5 steps, save, load, 4 more equal 9 uninterrupted bitwise (mu, Sigma, the moments of every latent, t, the ELBO); the same seed
    gives the same bits, another seed other ones"""
    AGP = env["AGP"]
    from agp_amd import nvi

    case = CS.VGP_CASES["logisticsoftmax-40-cla-adam"]
    a = _model(AGP, case)
    AGP.train_(a, 9)
    b = _model(AGP, case)
    AGP.train_(b, 5)
    AGP.save_trained_model(str(tmp_path / "m"), b)
    c = AGP.load_trained_model(str(tmp_path / "m"))
    assert repr(c.inference) == repr(a.inference) and repr(c.likelihood) == repr(a.likelihood) and c.inference.n_iter == 5
    assert (c.inference.nMC, c.inference.seed, c.inference.natural) == (CS.NMC, CS.SEED, False)
    AGP.train_(c, 4, state=True)
    assert all(np.array_equal(u, v) for u, v in zip(_full_state(a), _full_state(c)))
    assert nvi.get_opt_state(a)[2] == nvi.get_opt_state(c, latent=2)[2] == 9
    assert AGP.objective(a) == AGP.objective(c) == AGP.objective(a) and AGP.ELBO(a) == AGP.objective(a)
    assert a.nvi_alphas[5:] == c.nvi_alphas
    same, other = _model(AGP, case), _model(AGP, case, seed=CS.SEED + 1)
    AGP.train_(same, 9)
    AGP.train_(other, 9)
    assert all(np.array_equal(u, v) for u, v in zip(_full_state(a), _full_state(same)))
    assert not np.array_equal(a.get_state(0)[0], other.get_state(0)[0])


def test_svi_save_load_and_a_larger_batch(env, tmp_path):
    """MCIntegrationSVI: 5 steps, save, load, 4 more equal 9 uninterrupted bitwise; a handle re-created for a larger batch carries
    (mu, Sigma) and the optimiser state of every latent"""
    AGP = env["AGP"]
    case = CS.SPARSE_CASES["softmax-svi-cla-adam"]
    X, y, idx, a = _sparse_model(AGP, case)
    AGP.train_(a, X, y, 9, idx_stream=idx[:9])
    _, _, _, b = _sparse_model(AGP, case)
    AGP.train_(b, X, y, 5, idx_stream=idx[:5])
    AGP.save_trained_model(str(tmp_path / "s"), b)
    c = AGP.load_trained_model(str(tmp_path / "s"))
    assert repr(c.inference) == repr(a.inference) and c.inference.batchsize == CS.SPARSE["B"] and c.inference.seed == CS.SEED
    AGP.train_(c, X, y, 4, state=True, idx_stream=idx[5:9])
    assert all(np.array_equal(u, v) for u, v in zip(_full_state(a), _full_state(c)))
    before = _full_state(a)
    a._ensure_handle(len(X))
    assert all(np.array_equal(u, v) for u, v in zip(before, _full_state(a)))


# ---- 6. the single latent is untouched ---------------------------------------------------------------------------------------------
def test_single_latent_quadrature_is_bitwise_unchanged(env):
    """QuadratureVI, VGP, studentt-63-cla-adam (tests/_nvi_cases.py), 5 steps: mu, Sigma, the moments, t, the ELBO and the alphas
    equal, bit for bit, what the build before the per-latent state gave (recorded there into tests/golden/)"""
    AGP = env["AGP"]
    from agp_amd import nvi

    case = QCS.VGP_CASES["studentt-63-cla-adam"]
    X, y, mean = QCS.data(case)
    k = 1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(case["scale"]))
    inf = AGP.QuadratureVI(nGaussHermite=100, optimiser=AGP.ADAM(0.01), natural=False)
    model = AGP.VGP(X, y, k, agp_lik(AGP, case["lik"]), inf, optimiser=False, mean=mean)
    AGP.train_(model, 5)
    g = np.load(GOLDEN)
    mu, Sig = model.get_state(0)
    mm, ms, t = nvi.get_opt_state(model)
    for name, got in (("mu", mu), ("Sigma", Sig), ("mom_mu", mm), ("mom_sigma", ms)):
        assert np.array_equal(got, g[name]), name
    assert t == int(g["t"]) == 5 and AGP.objective(model) == float(g["elbo"]) and model.nvi_alphas == list(g["alphas"])
    assert all(isinstance(a, float) for a in model.nvi_alphas)


# ---- 7. the ABI ------------------------------------------------------------------------------------------------------------------------
def _handle(env, flags, lik, K, dtype=None, N=20, D=2, B=None):
    capi, torch = env["capi"], env["torch"]
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    d = capi.SvgpDesc()
    d.dtype = capi.F64 if dtype is None else dtype
    d.n_latent, d.latent_offset, d.stochastic = K, 0, 0
    d.m, d.D, d.max_batch = N, D, N if B is None else B
    d.lik = lik
    d.rm_kappa, d.rm_tau = 0.51, 1.0
    d.flags = flags
    h = C.c_void_p()
    st = L.agp_svgp_create(ctx, C.byref(d), C.byref(h))
    return L, ctx, h, st


def test_refusals_through_the_abi(env):
    capi, torch = env["capi"], env["torch"]
    FULL, NUM, MC = capi.FLAG_FULL, capi.FLAG_NUMERICAL, capi.FLAG_MC
    INV, UNS = 1, 5  # AGP_ERR_INVALID, AGP_ERR_UNSUPPORTED (include/agp_hip.h)
    sm3, lsm3 = capi.LikDesc(capi.LIK_SOFTMAX, 3, 0.0, 0.0), capi.LikDesc(capi.LIK_LOGISTICSOFTMAX, 3, 0.0, 0.0)

    def refused(flags, want, lik, K, **kw):
        L, ctx, h, st = _handle(env, flags, lik, K, **kw)
        assert st == want, (flags, K, kw, st)
        msg = L.agp_last_error(ctx).decode()
        L.agp_ctx_destroy(ctx)
        return msg

    for extra in (0, FULL):
        assert "AGP_FLAG_NUMERICAL" in refused(MC | extra, UNS, sm3, 3)                 # the flag alone
        refused(NUM | MC | extra, UNS, sm3, 3, dtype=capi.F32)
        assert "SoftMax" in refused(NUM | MC | extra, UNS, capi.LikDesc(capi.LIK_SOFTMAX, 1, 0.0, 0.0), 1)   # K = 1
        assert "SoftMax" in refused(NUM | MC | extra, UNS, capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0), 1)
        assert "SoftMax" in refused(NUM | MC | extra, UNS, capi.LikDesc(capi.LIK_LOGISTIC, 3, 0.0, 0.0), 3)
        assert "SoftMax" in refused(NUM | MC | extra, UNS, capi.LikDesc(capi.LIK_POISSON, 1, 2.0, 0.0), 1)
        refused(NUM | extra, UNS, sm3, 3)     # without the flag: the SoftMax likelihood does not exist, n_latent != 1 is refused
        assert "Logistic, StudentT and Laplace" in refused(NUM | extra, UNS, lsm3, 3)
    refused(0, UNS, sm3, 3)                   # ... nor on an AnalyticVI handle

    N, D, K = 20, 2, 3
    rng = np.random.default_rng(0)
    Xd = torch.as_tensor(rng.standard_normal((N, D)), device="cuda")
    yd = torch.as_tensor((np.arange(N) % K).astype(np.int32), device="cuda")
    x, w = np.polynomial.hermite.hermgauss(20)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vp = lambda t: C.c_void_p(t.data_ptr())

    L, ctx, h, st = _handle(env, NUM | MC | FULL, sm3, K, N=N, D=D)
    assert st == 0
    for k in range(K):
        assert L.agp_svgp_set_Z(h, k, vp(Xd), D) == 0
    step = lambda: L.agp_svgp_nvi_step(h, vp(Xd), D, vp(yd), None, N, 1.0)
    assert step() == INV and "agp_svgp_mcvi_configure" in L.agp_last_error(ctx).decode()       # nothing installed yet
    assert L.agp_svgp_nvi_configure(h, 20, dp(x), dp(w), 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == UNS
    assert "agp_svgp_mcvi_configure" in L.agp_last_error(ctx).decode()
    for bad in ((0, 1, capi.OPT_DESCENT, 0.1, 0.0), (65537, 1, capi.OPT_DESCENT, 0.1, 0.0), (50, 1, 7, 0.1, 0.0),
                (50, 1, capi.OPT_DESCENT, 0.0, 0.0), (50, 1, capi.OPT_MOMENTUM, 0.1, 1.5)):
        assert L.agp_svgp_mcvi_configure(h, bad[0], 11, bad[1], bad[2], bad[3], bad[4], 0.0, 0.0) == INV
    assert L.agp_svgp_mcvi_configure(h, 50, 11, 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == 0
    assert L.agp_svgp_cavi_step(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert L.agp_svgp_step_local(h, vp(Xd), D, vp(yd), None, N, 1.0) == UNS
    assert L.agp_svgp_hyper_step(h) == UNS
    dv, ds = C.c_double(), (C.c_double * D)()
    assert L.agp_svgp_hypergrad(h, 0, C.byref(dv), ds, None) == UNS
    assert L.agp_svgp_prefetch(h, vp(Xd), D, None, N) == UNS
    assert step() == 0
    a, hv, rj = C.c_double(), C.c_int64(), C.c_int64()
    for k in range(K):
        assert L.agp_svgp_nvi_info(h, k, C.byref(a), C.byref(hv), C.byref(rj)) == 0 and 0 < a.value <= 1
    assert L.agp_svgp_nvi_info(h, K, C.byref(a), C.byref(hv), C.byref(rj)) == INV
    assert L.agp_svgp_nvi_info(h, -1, C.byref(a), C.byref(hv), C.byref(rj)) == INV
    mu = torch.empty(N, dtype=torch.float64, device="cuda")
    assert L.agp_svgp_get_state(h, K, vp(mu), None, None, None) == INV
    assert L.agp_svgp_get_state(h, K - 1, vp(mu), None, None, None) == 0
    assert L.agp_svgp_check_status(h) == 0
    bad_y = torch.full((N,), K, dtype=torch.int32, device="cuda")     # a class index outside [0, K) is latched
    assert L.agp_svgp_nvi_step(h, vp(Xd), D, vp(bad_y), None, N, 1.0) == 0
    assert L.agp_svgp_check_status(h) == 6  # AGP_ERR_LABELS
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx)

    L, ctx, h, st = _handle(env, NUM | FULL, capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0), 1, N=N, D=D)   # a quadrature handle
    assert st == 0
    assert L.agp_svgp_mcvi_configure(h, 50, 11, 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == UNS
    assert "agp_svgp_nvi_configure" in L.agp_last_error(ctx).decode()
    L.agp_svgp_destroy(h)
    L, ctx2, h, st = _handle(env, FULL, capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0), 1, N=N, D=D)        # an AnalyticVI handle
    assert st == 0 and L.agp_svgp_mcvi_configure(h, 50, 11, 1, capi.OPT_DESCENT, 0.1, 0.0, 0.0, 0.0) == UNS
    L.agp_svgp_destroy(h)
    L.agp_ctx_destroy(ctx2)

    ell, g = torch.empty(N, dtype=torch.float64, device="cuda"), torch.zeros(K, N, dtype=torch.float64, device="cuda")
    call = lambda lik, K_, nMC=10, y=yd: L.agp_mc_expectations(ctx, C.byref(lik), vp(y), vp(g), vp(g), N, K_, nMC, 3, 1, 2, vp(ell),
                                                                vp(torch.empty_like(g)), vp(torch.empty_like(g)))
    assert call(sm3, K) == 0
    assert call(capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0), K) == UNS and call(sm3, 2) == UNS
    assert call(capi.LikDesc(capi.LIK_SOFTMAX, 65, 0.0, 0.0), 65) == UNS
    assert call(sm3, K, nMC=0) == INV and call(sm3, K, nMC=65537) == INV
    assert call(sm3, K, y=bad_y) == 6
    assert L.agp_mc_normals(ctx, 3, -1, 2, 10, K, vp(g)) == INV and L.agp_mc_normals(ctx, 3, 1, 2, 0, K, vp(g)) == INV
    L.agp_ctx_destroy(ctx)


def test_sparse_step_with_pitched_x(env):
    """the sparse step reads (x, ldx): contiguous and NaN-guarded pitched x in every layout give the same bits for every latent,
    guards intact"""
    AGP, torch = env["AGP"], env["torch"]
    case = CS.SPARSE_CASES["logisticsoftmax-svi-nat-descent"]
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
        results.append(_full_state(model) + [np.array(out.value)])
    for r in results[1:]:
        assert all(np.array_equal(u, w) and np.all(np.isfinite(u)) for u, w in zip(r, results[0]))
