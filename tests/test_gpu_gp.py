"""GP (exact regression, Analytic()) on the MI355X against the NumPy restatement tests/_gp_ref.py, in both elbo modes: the
constructor's iteration, 10-iteration trajectories across the Cholesky drivers (single tile, task graph, per column, blocked, the
in-stream fallback), kernels, prior means, the hyper step, predictions, persistence, a large N and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = 5  # AGP_ERR_UNSUPPORTED
KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel", "matern32": "Matern32Kernel",
           "exponential": "ExponentialKernel"}


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


def _case(env, N, D=3, seed=5, kind="sqexponential", scale=2.0, mean=None, mode="corrected", optimiser=False, noise=0.05,
          opt_noise=True):
    """the kernel is 1.5 * kind o transform on both sides; mean: None, a number or N numbers"""
    from _gp_ref import GPRef

    AGP, R = env["AGP"], env["R"]
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7 + 0.1 * rng.standard_normal(N)
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(scale)
    k = 1.5 * (getattr(AGP, KERNELS[kind])() @ tr)
    model = AGP.GP(X, y, k, noise=noise, opt_noise=opt_noise, optimiser=optimiser, mean=mean, elbo_mode=mode)
    rscale = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64).copy()
    ropt = None if optimiser is False else R.Adam(optimiser.eta)
    ref = GPRef(R.Kernel(kind, rscale, 1.5), X, y, noise=noise, opt_noise=opt_noise, mu0=mean, mode=mode, optimiser=ropt)
    return X, y, model, ref


def _check(model, ref, tol=1e-8):
    import agp_amd as AGP

    alpha, Sig = model.get_state()
    assert _rel(alpha, ref.alpha) < tol
    assert _rel(Sig, ref.Sigma) < tol
    assert abs(AGP.ELBO(model) - ref.logp) < tol * max(1.0, abs(ref.logp))
    assert abs(model.likelihood.sigma2 - ref.sigma2) < tol * ref.sigma2


def _traj(env, model, ref, its=10):
    """train one iteration at a time (a state carried on) and compare the log p and sigma2 trajectories, then the posterior"""
    AGP = env["AGP"]
    lps = []
    AGP.train_(model, its, callback=lambda m, s, n: lps.append(AGP.objective(m)))
    ref.train(its)
    assert np.max(np.abs(np.array(lps) - np.array(ref.logp_trace[-its:]))) < 1e-8 * max(1.0, np.max(np.abs(lps)))
    _check(model, ref)


def test_gp_reference_behaviour(env):
    """test/likelihood/gaussian.jl:15-35 verbatim: N = 20, d = 2, SE o ScaleTransform(10), sigma = 0.1"""
    AGP = env["AGP"]
    rng = np.random.default_rng(42)
    N, d, sigma = 20, 2, 0.1
    X = rng.random((N, d))
    k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(10.0)
    Kx = np.exp(-0.5 * 100.0 * np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)) + 1e-4 * np.eye(N)
    f = np.linalg.cholesky(Kx) @ rng.standard_normal(N)
    y = f + sigma * rng.standard_normal(N)
    model = AGP.GP(X, y, k, opt_noise=True)
    assert repr(model).startswith("Gaussian Process with a Gaussian likelihood") and repr(model).endswith("Analytic Inference ")
    l0 = AGP.ELBO(model)
    AGP.train_(model, 10)
    assert AGP.ELBO(model) > l0
    mu, var = AGP.proba_y(model, X)
    assert np.all(var > 0)


@pytest.mark.parametrize("mode", ["corrected", "reference"])
def test_gp_constructor(env, mode):
    X, y, model, ref = _case(env, 50, mode=mode)
    assert model.inference.n_iter == 1
    assert model.likelihood.sigma2 != 0.05
    _check(model, ref)


@pytest.mark.parametrize("mode", ["corrected", "reference"])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 200, 2049, 6017])
def test_gp_parity(env, N, mode):
    X, y, model, ref = _case(env, N, mode=mode, seed=N)
    _traj(env, model, ref)
    Xt = np.vstack([X[: min(N, 5)], np.random.default_rng(1).random((7, X.shape[1]))])
    _check_predictions(env, model, ref, Xt)


@pytest.mark.parametrize("kind,scale", [("sqexponential", [1.5, 2.5, 1.0]), ("matern52", 2.0), ("matern32", 2.0),
                                        ("matern52", [1.5, 2.5, 1.0]), ("matern32", [1.5, 2.5, 1.0])])
def test_gp_kernels_hyper(env, kind, scale):
    """hypergrad against the restatement (itself checked against autograd and scikit-learn on the host), then the kernel and sigma2
    trajectory with ADAM over 10 iterations"""
    AGP = env["AGP"]
    X, y, model, ref = _case(env, 120, kind=kind, scale=scale, optimiser=AGP.ADAM(0.01))
    dv, ds = model.hypergrad()
    rv, rs = ref.hyper_grad()
    assert abs(dv - rv) < 1e-8 * max(1.0, abs(rv))
    assert _rel(ds, rs) < 1e-8
    _traj(env, model, ref)
    kr = model.kernels[0]
    assert abs(kr.variance - ref.kernel.sigma2) < 1e-8 * ref.kernel.sigma2
    assert kr.variance != 1.5


def test_gp_exponential_hypergrad_refused(env):
    X, y, model, ref = _case(env, 70, kind="exponential")
    dv, ds = C.c_double(), (C.c_double * 3)()
    assert env["capi"].lib().agp_svgp_hypergrad(model._h, 0, C.byref(dv), ds, None) == 5


def test_gp_reference_mode_kernel_frozen(env):
    AGP = env["AGP"]
    X, y, model, ref = _case(env, 90, mode="reference", optimiser=AGP.ADAM(0.01))
    with pytest.warns(UserWarning, match="Kernel gradients are equal to zero"):
        AGP.train_(model, 10)
    ref.train(10)
    assert model.kernels[0].variance == 1.5 and model.kernels[0].transform.s == 2.0
    _check(model, ref)


@pytest.mark.parametrize("mode", ["corrected", "reference"])
@pytest.mark.parametrize("mean", [0.7, "vec"])
def test_gp_means(env, mode, mean):
    N = 130
    mu0 = 0.7 if mean == 0.7 else np.linspace(-0.5, 0.5, N)
    X, y, model, ref = _case(env, N, mean=mu0, mode=mode)
    _traj(env, model, ref)
    _check_predictions(env, model, ref, X[:9])


def _check_predictions(env, model, ref, Xt):
    AGP = env["AGP"]
    mu, var, cov = ref.predict_f(Xt)
    mf, vf = AGP.predict_f(model, Xt, cov=True)
    assert _rel(mf, mu) < 1e-8
    assert _rel(AGP.predict_f(model, Xt), mu) < 1e-8
    assert _rel(AGP.predict_y(model, Xt), mu) < 1e-8
    # var* = k** + jitt - ks' Sigma^-1 ks cancels terms of size S = max_i |ks_i|' |Sigma^-1| |ks_i|; each side's Sigma^-1 carries a
    # rounding of ~eps cond_1(Sigma) relative to its entries, so the two agree to about eps cond_1(Sigma) S in absolute terms
    Ks = ref.kernel.matrix(Xt, ref.X)
    S = np.max(np.einsum("ij,jk,ik->i", np.abs(Ks), np.abs(ref.Sinv), np.abs(Ks)))
    cond = np.max(np.sum(np.abs(ref.Sigma), axis=0)) * np.max(np.sum(np.abs(ref.Sinv), axis=0))
    tol = max(1e-8, np.finfo(np.float64).eps * cond * S / np.max(np.abs(var)))
    assert _rel(vf, var) < tol
    m2, c2 = AGP.predict_f(model, Xt, cov=True, diag=False)
    assert _rel(m2, mu) < 1e-8 and _rel(c2, cov) < tol
    pm, pv = AGP.proba_y(model, Xt)
    assert _rel(pm, mu) < 1e-8 and _rel(pv, var + ref.sigma2) < tol


def test_gp_persistence(env, tmp_path):
    AGP = env["AGP"]
    X, y, model, ref = _case(env, 80, optimiser=AGP.ADAM(0.01), mean=0.3)
    AGP.train_(model, 5)
    Xt = np.random.default_rng(2).random((11, 3))
    f = str(tmp_path / "gp.npz")
    AGP.save_trained_model(f, model)
    m2 = AGP.load_trained_model(f)
    assert type(m2).__name__ == "GP" and m2.inference.n_iter == model.inference.n_iter
    assert m2.likelihood.sigma2 == model.likelihood.sigma2 and m2.kernels[0].variance == model.kernels[0].variance
    a, b = AGP.proba_y(model, Xt), AGP.proba_y(m2, Xt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert AGP.ELBO(m2) == AGP.ELBO(model)


def test_gp_large(env):
    """N = 16384: finite, and Sigma alpha = r to 1e-8 with Sigma = K + (jitt + sigma2) I formed on the host from X and the kernel, in
    row blocks (no host factorisation).  A solve that is rounded rather than wrong leaves ~eps ||Sigma|| ||alpha|| <= eps N / sigma2
    ||y|| ~ 2e-10 ||y||; a wrong device kernel matrix or factor leaves O(1)."""
    AGP, R = env["AGP"], env["R"]
    rng = np.random.default_rng(7)
    N, D = 16384, 16
    X = rng.random((N, D))
    y = np.sin(3 * X[:, 0]) + X[:, 1] - 0.5 + 0.1 * rng.standard_normal(N)
    model = AGP.GP(X, y, AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5), noise=0.01, optimiser=False)
    AGP.train_(model, 3)
    alpha, _ = model.get_state()
    assert np.all(np.isfinite(alpha)) and np.isfinite(AGP.ELBO(model))
    ker, s2 = R.Kernel("sqexponential", 0.5, 1.0), model.likelihood.sigma2
    Sa = np.empty(N)
    for r0 in range(0, N, 1024):
        Sa[r0:r0 + 1024] = ker.matrix(X[r0:r0 + 1024], X) @ alpha
    Sa += (1e-4 + s2) * alpha
    assert np.linalg.norm(Sa - y) / np.linalg.norm(y) < 1e-8


def test_gp_reference_mode_hyper_apply(env):
    """the reference mode steps nothing, also when the caller supplies a gradient (agp_svgp_hyper_apply); the corrected mode does"""
    AGP, capi = env["AGP"], env["capi"]
    L = capi.lib()
    for mode, moves in (("reference", False), ("corrected", True)):
        X, y, model, ref = _case(env, 60, mode=mode, optimiser=AGP.ADAM(0.01))
        dv, ds = C.c_double(0.5), (C.c_double * 3)(0.5, 0.5, 0.5)
        assert L.agp_svgp_hyper_apply(model._h, 0, C.byref(dv), ds, None) == 0
        var, sc = C.c_double(), (C.c_double * 3)()
        assert L.agp_svgp_get_kernel(model._h, 0, C.byref(var), sc) == 0
        assert (var.value != 1.5) == moves and (sc[0] != 2.0) == moves


def test_gp_refusals(env):
    AGP, capi = env["AGP"], env["capi"]
    L = capi.lib()
    X, y, model, ref = _case(env, 40)
    h = model._h
    e1 = (C.c_double * 40)()
    assert L.agp_svgp_get_state(h, 0, None, None, e1, None) == UNSUPPORTED
    assert L.agp_svgp_set_state(h, 0, e1, e1) == UNSUPPORTED
    assert L.agp_svgp_step_local(h, None, 3, None, None, 40, 1.0) == UNSUPPORTED
    assert L.agp_svgp_prefetch(h, None, 3, None, 40) == UNSUPPORTED
    assert L.agp_svgp_set_batch_shard(h, 0, 2) == UNSUPPORTED
    out = (C.c_double * 3)()
    assert L.agp_svgp_elbo_terms(h, out) == UNSUPPORTED
    with pytest.raises(ValueError, match="Gaussian Likelihood you should directly use the `GP` model"):
        AGP.VGP(X, y, AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI())
    # agp_svgp_create's refusals of exact descriptors (Logistic unless lik is given): the generic latent count answers first and
    # writes no message; the exact model's check comes before the full model's
    from test_gpu_vgp import create_status

    G, FE = capi.LikDesc(capi.LIK_GAUSSIAN, 1, 0.05, 0.0), capi.FLAG_FULL | capi.FLAG_EXACT
    for fields, status, msg in [(dict(flags=capi.FLAG_EXACT, lik=G), 5, "exact GP regression is a full model"),
                                (dict(flags=FE), 5, "one latent and a Gaussian likelihood"),
                                (dict(flags=FE, max_batch=32), 5, "one latent and a Gaussian likelihood"),
                                (dict(flags=FE, lik=G, n_latent=2), 1, None),
                                (dict(flags=FE, lik=G, max_batch=32), 1, "max_batch = m = N")]:
        st, err = create_status(capi, **fields)
        assert st == status and (msg in err if msg else err == ""), (fields, st, err)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import agp_amd as AGP
from agp_amd import capi
import ctypes as C
from oracle import agp_ref as R
from _gp_ref import GPRef
N = {N}
rng = np.random.default_rng(N)
X = rng.random((N, 3))
y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7 + 0.1 * rng.standard_normal(N)
m = AGP.GP(X, y, 1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0)), noise=0.05, optimiser=False)
ref = GPRef(R.Kernel("sqexponential", 2.0, 1.5), X, y, noise=0.05)
AGP.train_(m, 10); ref.train(10)
a, S = m.get_state()
rel = lambda u, v: float(np.max(np.abs(u - v)) / np.max(np.abs(v)))
assert rel(a, ref.alpha) < 1e-8 and rel(S, ref.Sigma) < 1e-8, (rel(a, ref.alpha), rel(S, ref.Sigma))
assert abs(AGP.ELBO(m) - ref.logp) < 1e-8 * abs(ref.logp) and abs(m.likelihood.sigma2 - ref.sigma2) < 1e-8 * ref.sigma2
n = C.c_int64()
assert capi.lib().agp_ctx_task_graph_fallbacks(m._ctx, C.byref(n)) == 0
print("FALLBACKS", n.value)
"""


def _child(extra_env, N):
    env_ = dict(os.environ, **extra_env)
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), N=N)
    p = subprocess.run([sys.executable, "-c", code], env=env_, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return int(p.stdout.split("FALLBACKS")[1].split()[0])


def test_gp_per_column_driver(env):
    _child({"AGP_CHOL_DAG": "0"}, 1000)


def test_gp_task_graph_fallback(env):
    """a lost task-graph dependency (forced): the in-stream fallback rebuilds Sigma from K and the sigma2 word"""
    import _knobs as K_

    n = _child({"AGP_DAG_TEST_ABORT": "1"}, 1000)  # (nt = 16: the task-graph driver; N = 2049 already takes per-column launches)
    assert n > 0 or K_.no_task_graph()
