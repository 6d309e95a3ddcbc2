"""VGP (the full variational GP, AGP_FLAG_FULL handle) on the MI355X against the NumPy restatement tests/_vgp_ref.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from _liks import agp_lik, labels, oracle_lik

pytestmark = pytest.mark.gpu

LIKS = ["logistic", "studentt", "logisticsoftmax", "laplace", "bayesiansvm", "poisson", "negbinomial", "heteroscedastic"]


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

    return dict(AGP=AGP, capi=capi, R=R)


KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel", "matern32": "Matern32Kernel",
           "exponential": "ExponentialKernel"}


def _case(env, likname, N, D=3, seed=3, optimiser=False, mean=None, kind="sqexponential", scale=2.0):
    """kind: a KERNELS key; scale: a number (ScaleTransform) or D numbers (ARDTransform); mean: None, a number (ConstantMean) or
    N numbers (EmpiricalMean).  The kernel is 1.5 * kind o transform on both sides."""
    from _vgp_ref import VGPRef

    AGP, R = env["AGP"], env["R"]
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7
    y = labels(likname, f, X, rng)
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(scale)
    k = 1.5 * (getattr(AGP, KERNELS[kind])() @ tr)
    model = AGP.VGP(X, y, k, agp_lik(AGP, likname), AGP.AnalyticVI(), optimiser=optimiser, mean=mean)
    lr = oracle_lik(R, likname)
    mu0 = None if mean is None else np.full(N, mean) if np.isscalar(mean) else np.asarray(mean, dtype=np.float64)
    rscale = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64).copy()
    ref = VGPRef(R.Kernel(kind, rscale, 1.5), lr, X, mu0=mu0)
    return X, R.treat_labels(y, lr), model, ref


def _check_state(env, model, ref, yt, tol=1e-8):
    capi = env["capi"]
    for k in range(model.n_latent):
        mu, Sig, e1, e2 = model.get_state(k)
        assert _rel(e1, ref.eta1[k]) < tol
        assert _rel(e2, ref.eta2[k]) < tol
        assert _rel(mu, ref.mu[k]) < tol
        assert _rel(Sig, ref.Sigma[k]) < tol
    n, lv = len(yt), ref.lv
    if ref.lik.name == "logisticsoftmax":  # the multi-latent local state: per latent c, gamma, theta; alpha shared
        for k in range(model.n_latent):
            assert _rel(model.get_matrix(capi.VEC_C, k, n), lv["c"][k]) < tol
            assert _rel(model.get_matrix(capi.VEC_GAMMA, k, n), lv["gamma"][k]) < tol
            assert _rel(model.get_matrix(capi.VEC_THETA, k, n), lv["theta"][k]) < tol
        assert _rel(model.get_matrix(capi.VEC_ALPHA, 0, n), lv["alpha"]) < tol
    elif ref.lik.name == "heteroscedastic":  # latent 0 -> phi, gamma ; latent 1 -> c, sigg (agp_hip.h AGP_VEC_*) ; lambda
        assert _rel(model.get_matrix(capi.VEC_C, 0, n), lv["phi"]) < tol
        assert _rel(model.get_matrix(capi.VEC_C, 1, n), lv["c"]) < tol
        assert _rel(model.get_matrix(capi.VEC_GAMMA, 0, n), lv["gamma"]) < tol
        assert _rel(model.get_matrix(capi.VEC_GAMMA, 1, n), lv["sigg"]) < tol
        assert _rel(model.get_matrix(capi.VEC_THETA, 1, n), lv["theta"]) < tol
    else:
        assert _rel(model.get_matrix(capi.VEC_THETA, 0, n), lv["theta"]) < tol
    ea, er = env["AGP"].objective(model), ref.elbo(yt)
    assert abs(ea - er) < tol * max(1.0, abs(er)), (ea, er)


@pytest.mark.parametrize("likname", LIKS)
@pytest.mark.parametrize("N", [173, 200])
def test_vgp_parity(env, likname, N):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, likname, N)
    done = 0
    for it in (1, 2, 10):
        AGP.train_(model, it - done, state=None if done == 0 else True)
        for _ in range(it - done):
            ref.step(yt)
        done = it
        _check_state(env, model, ref, yt)
    if hasattr(ref.lik, "lam"):
        assert model.likelihood.lam == pytest.approx(ref.lik.lam, rel=1e-10)


@pytest.mark.parametrize("N", [2048, 4100])
def test_vgp_parity_large(env, N):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "logistic", N, seed=5)
    AGP.train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    _check_state(env, model, ref, yt)


def test_vgp_parity_without_task_graph(built):
    code = ("import sys; sys.path.insert(0, 'tests'); import numpy as np; import test_gpu_vgp as T; "
            "from oracle import agp_ref as R; import agp_amd as AGP; from agp_amd import capi; "
            "env = dict(AGP=AGP, capi=capi, R=R); X, yt, m, ref = T._case(env, 'logistic', 1000, seed=9); "
            "AGP.train_(m, 3); [ref.step(yt) for _ in range(3)]; T._check_state(env, m, ref, yt); print('OK')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, AGP_CHOL_DAG="0"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("likname", ["logistic", "poisson", "heteroscedastic", "logisticsoftmax"])
def test_vgp_predictions(env, likname):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, likname, 150)
    AGP.train_(model, 4)
    for _ in range(4):
        ref.step(yt)
    Xt = np.random.default_rng(1).random((57, 3))
    mus, vars_, covs = ref.predict_f(Xt)
    # (variances: k** - diag(K*n A Kn*) cancels the digits of A's O(cond K) entries; the SVGP parity tests use the same bound)
    if model.n_latent == 1:
        mf, vf = AGP.predict_f(model, Xt, cov=True)
        assert _rel(mf, mus[0]) < 1e-8 and _rel(vf, vars_[0]) < 1e-6
        mc, cc = AGP.predict_f(model, Xt, cov=True, diag=False)
        assert _rel(mc, mus[0]) < 1e-8 and _rel(cc, covs[0]) < 1e-6
        from oracle import agp_ref as R

        pa = AGP.proba_y(model, Xt)
        pr = R.compute_proba(ref.lik, (mus[0],), (vars_[0],))
        assert _rel(pa[0], pr[0]) < 1e-8 and _rel(pa[1], pr[1]) < 1e-6
        py = AGP.predict_y(model, Xt)
        if likname == "logistic":
            assert np.array_equal(np.asarray(py), mus[0] > 0)
        else:
            assert _rel(py, ref.lik.lam / (1 + np.exp(-mus[0]))) < 1e-8
    else:
        mf, vf = AGP.predict_f(model, Xt, cov=True)
        for k in range(model.n_latent):
            assert _rel(mf[k], mus[k]) < 1e-8 and _rel(vf[k], vars_[k]) < 1e-6


def test_vgp_hypergrad_matches_autograd(env):
    import torch
    from _torch_elbo import kernel_matrix

    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "logistic", 120, mean=0.3)
    AGP.train_(model, 3)
    dvar, dscale = model.hypergrad(0)
    mu, Sig, _, _ = model.get_state(0)
    mu = mu - 0.3  # d = mu - mu0
    Xt = torch.tensor(X)
    s = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    v = torch.tensor(1.5, dtype=torch.float64, requires_grad=True)
    K = kernel_matrix("sqexponential", Xt, Xt, s, v) + 1e-4 * torch.eye(len(X), dtype=torch.float64)
    Lk = torch.linalg.cholesky(K)
    S, m = torch.tensor(Sig), torch.tensor(mu)
    kl = 0.5 * (2 * torch.log(torch.diagonal(Lk)).sum() - torch.logdet(S) + torch.trace(torch.cholesky_solve(S, Lk))
                + (m @ torch.cholesky_solve(m[:, None], Lk))[0] - len(X))
    (-kl).backward()
    # (both sides sum products of K^-1's O(cond K) entries into an O(1) gradient: agreement to 1e-6 of the result)
    assert dvar == pytest.approx(v.grad.item(), rel=1e-6)
    assert float(np.sum(dscale)) == pytest.approx(s.grad.item(), rel=1e-6)


def test_vgp_hyper_trajectory(env):
    """the default ADAM(0.01) hyper step inside train!: kernel parameters, posterior and ELBO over 8 iterations (hyper steps after
    iterations 4..7) against the restatement's train loop"""
    from oracle import agp_ref as R

    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "logistic", 180, optimiser=True)
    assert model.k_opt.eta == 0.01
    elbos = []
    AGP.train_(model, 8, callback=lambda m, s, i: elbos.append(AGP.objective(m)))
    elbos_r = []
    ref.train(yt, 8, opt=R.Adam(0.01), callback=lambda r: elbos_r.append(r.elbo(yt)))
    k = model.kernels[0]
    assert ref.kernel.sigma2 != 1.5 and ref.kernel.scale != 2.0  # the kernel did move
    assert k.variance == pytest.approx(ref.kernel.sigma2, rel=1e-9)
    assert float(k.transform.s) == pytest.approx(ref.kernel.scale, rel=1e-9)
    assert np.allclose(elbos, elbos_r, rtol=1e-8, atol=1e-8), (elbos, elbos_r)
    ref.refresh_K()
    _check_state(env, model, ref, yt, tol=1e-7)


def test_vgp_save_load_round_trip(env, tmp_path):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "poisson", 140, optimiser=True)
    AGP.train_(model, 5)
    f = str(tmp_path / "vgp.npz")
    AGP.save_trained_model(f, model)
    m2 = AGP.load_trained_model(f)
    assert isinstance(m2, AGP.VGP) and m2.N == model.N
    Xt = np.random.default_rng(4).random((31, 3))
    a, b = AGP.predict_f(model, Xt, cov=True), AGP.predict_f(m2, Xt, cov=True)
    assert _rel(b[0], a[0]) < 1e-10 and _rel(b[1], a[1]) < 1e-8
    assert m2.likelihood.lam == pytest.approx(model.likelihood.lam, rel=1e-12)
    for q in (model, m2):  # both go on training identically (posterior, kernel, optimiser moments and lambda travelled)
        AGP.train_(q, 3, state=True)
    for u, v in zip(model.get_state(0), m2.get_state(0)):
        assert _rel(v, u) < 1e-10


def test_vgp_elbo_after_set_state(env):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "logistic", 160)
    AGP.train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    mu, Sig, e1, e2 = model.get_state(0)
    e2b = e2 - 0.05 * np.eye(len(X))
    model.set_state(0, e1, e2b)
    ref.eta2[0] = e2b
    ref.mu[0], ref.Sigma[0] = env["R"].natural_to_standard(e1, e2b)
    ea, er = AGP.ELBO(model), ref.elbo_fresh(yt)
    assert abs(ea - er) < 1e-8 * max(1.0, abs(er)), (ea, er)


def test_vgp_refusals_and_unsupported(env):
    AGP, capi = env["AGP"], env["capi"]
    X = np.random.default_rng(0).random((64, 2))
    y = (X[:, 0] > 0.5).astype(int)
    k = AGP.SqExponentialKernel()
    with pytest.raises(ValueError, match="Gaussian Likelihood"):
        AGP.VGP(X, X[:, 0], k, AGP.GaussianLikelihood(0.1), AGP.AnalyticVI())
    with pytest.raises(ValueError):
        AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(10))
    with pytest.raises(NotImplementedError):
        AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), T=np.float32)
    m = AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(m, 2)
    L, h = capi.lib(), m._h
    assert L.agp_svgp_step_stats(h) == 5
    assert L.agp_svgp_step_global(h) == 5
    assert L.agp_svgp_set_batch_shard(h, 0, 2) == 5
    assert L.agp_svgp_prefetch(h, None, 2, None, 64) == 5
    assert L.agp_svgp_elbo_multi(h, None, 0, C.byref(C.c_double())) == 5
    n0 = C.c_int64()
    L.agp_svgp_step_counters(h, C.byref(n0), C.byref(C.c_int64()))
    assert L.agp_svgp_cavi_step_multi(h, None, 0, None, 2, None, None, 64, 1.0) == 5
    assert L.agp_svgp_hyper_step_multi(h, None, 0) == 5
    n1 = C.c_int64()
    L.agp_svgp_step_counters(h, C.byref(n1), C.byref(C.c_int64()))
    assert n1.value == n0.value  # refused before anything was counted or enqueued
    dZ = C.c_void_p(1)
    assert L.agp_svgp_hyper_apply(h, 0, None, None, dZ) == 5
    dv = C.c_double()
    assert L.agp_svgp_hypergrad(h, 0, C.byref(dv), None, dZ) == 5
    # nothing changed: the model still trains
    AGP.train_(m, 1, state=True)
    assert np.isfinite(AGP.objective(m))
    # agp_svgp_create refuses these full descriptors; the generic checks (here nu) answer before the full model's own
    G, ST = capi.LikDesc(capi.LIK_GAUSSIAN, 1, 0.1, 0.0), capi.LikDesc(capi.LIK_STUDENTT, 1, 0.4, 1.0)
    for fields, status, msg in [(dict(dtype=capi.F32), 5, "the full model is Float64 only"),
                                (dict(stochastic=1, rm_kappa=0.75, rm_tau=1.0), 1, "max_batch = m = N"),
                                (dict(max_batch=32), 1, "max_batch = m = N"),
                                (dict(latent_offset=1), 1, "max_batch = m = N"),
                                (dict(lik=G), 5, "Gaussian Likelihood you should directly use the `GP` model"),
                                (dict(lik=G, max_batch=32), 1, "max_batch = m = N"),
                                (dict(lik=ST, max_batch=32), 1, "nu should be greater than 0.5")]:
        st, err = create_status(capi, **fields)
        assert st == status and msg in err, (fields, st, err)


def create_status(capi, **fields):
    """agp_svgp_create on a fresh context with a 64-point Logistic VGP descriptor, `fields` set on top -> (status, agp_last_error)"""
    import torch

    L = capi.lib()
    ctx, h = C.c_void_p(), C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        d = capi.SvgpDesc(dtype=capi.F64, n_latent=1, m=64, D=2, max_batch=64, lik=capi.LikDesc(capi.LIK_LOGISTIC, 1, 0.0, 0.0),
                          flags=capi.FLAG_FULL)
        for k, v in fields.items():
            setattr(d, k, v)
        st = L.agp_svgp_create(ctx, C.byref(d), C.byref(h))
        if h.value:
            L.agp_svgp_destroy(h)
        return st, L.agp_last_error(ctx).decode()
    finally:
        L.agp_ctx_destroy(ctx)


def test_vgp_8192(env):
    AGP = env["AGP"]
    rng = np.random.default_rng(11)
    N = 8192
    X = rng.random((N, 16))
    y = (np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 > 0).astype(int)
    k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
    m = AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    elbos = []
    AGP.train_(m, 6, callback=lambda mm, s, i: elbos.append(AGP.objective(mm)))
    assert all(np.isfinite(elbos))
    assert all(b >= a - 1e-8 * abs(a) for a, b in zip(elbos, elbos[1:])), elbos
    n = C.c_int64()
    env["capi"].lib().agp_ctx_task_graph_fallbacks(m._ctx, C.byref(n))
    assert n.value == 0


@pytest.mark.parametrize("name", ["studentt", "laplace", "heteroscedastic", "logistic", "bayesiansvm", "logisticsoftmax", "poisson",
                                  "negativebinomial"])
def test_vgp_rows_of_the_reference_likelihood_suite(env, name):
    """test_inference_VGP (test/testingtools.jl:255-270) for the likelihoods whose test file marks "VGP" => "AVI" => true, with the
    reference's data (make_case) and call sequence (run_tests); Gaussian is refused (VGP.jl:54-56)."""
    import copy

    from test_gpu_reference_suite import make_case, run_tests

    AGP = env["AGP"]
    rng = np.random.default_rng(42)
    X, f, y, lik, problem, var = make_case(AGP, name, rng)
    kern = lambda: var * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(10.0))  # noqa: E731
    model = AGP.VGP(X, y, kern(), copy.deepcopy(lik), AGP.AnalyticVI(), optimiser=False)
    assert AGP.n_latent(model) == (3 if name == "logisticsoftmax" else 2 if name == "heteroscedastic" else 1)
    assert model.T == np.dtype(np.float64) and model.likelihood is not lik
    model_opt = AGP.VGP(X, y, kern(), copy.deepcopy(lik), AGP.AnalyticVI(), optimiser=True)
    run_tests(AGP, model, model_opt, X, f, y, problem)


def test_vgp_gaussian_row_is_refused(env):
    from test_gpu_reference_suite import make_case

    AGP = env["AGP"]
    X, f, y, lik, problem, var = make_case(AGP, "gaussian", np.random.default_rng(42))
    with pytest.raises(ValueError, match="Gaussian Likelihood"):
        AGP.VGP(X, y, AGP.SqExponentialKernel(), lik, AGP.AnalyticVI(), optimiser=False)
