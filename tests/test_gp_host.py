"""GP on the host: the NumPy restatement tests/_gp_ref.py against scikit-learn's exact GP regression and torch autograd, the
reference mode's three defects (G1 - G3), the constructor's refusals and the ABI / shim surface of the model."""
import os
import re
import warnings

import numpy as np
import pytest

from _gp_ref import GPRef
from oracle import agp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITT = 1e-4


def _data(N=40, D=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7 + 0.1 * rng.standard_normal(N)
    return X, y


def _ref(kind, scale, X, y, s2=0.05, mode="corrected", mu0=None):
    return GPRef(R.Kernel(kind, scale, 1.7), X, y, noise=s2, opt_noise=False, mode=mode, mu0=mu0, construct=False)


def _grad_log(ref):
    """(d log p / d log variance, d log p / d log scales, d log p / d log(jitt + sigma2)) of the restatement"""
    gv, gs = ref.hyper_grad()
    s = np.atleast_1d(np.asarray(ref.kernel.scale, dtype=np.float64))
    gs = np.array([np.sum(gs)]) if np.isscalar(ref.kernel.scale) else gs
    return np.concatenate([[ref.kernel.sigma2 * gv], s * gs, [(JITT + ref.sigma2) * ref.noise_grad()]])


@pytest.mark.parametrize("kind", ["sqexponential", "matern52", "matern32"])
@pytest.mark.parametrize("scale", [2.0, [1.5, 2.5, 0.8]])
def test_gp_ref_against_sklearn(kind, scale):
    gpk = pytest.importorskip("sklearn.gaussian_process.kernels")
    from sklearn.gaussian_process import GaussianProcessRegressor

    X, y = _data()
    sc = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64)
    ref = _ref(kind, sc, X, y)
    ell = 1.0 / np.asarray(sc, dtype=np.float64)
    base = gpk.RBF(ell) if kind == "sqexponential" else gpk.Matern(ell, nu=2.5 if kind == "matern52" else 1.5)
    k = gpk.ConstantKernel(1.7) * base + gpk.WhiteKernel(JITT + ref.sigma2)
    gpr = GaussianProcessRegressor(k, alpha=0.0, optimizer=None).fit(X, y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lml, grad = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
    assert abs(lml - ref.logp) < 1e-10 * abs(lml)
    ours = _grad_log(ref)
    ours[1:-1] *= -1.0  # theta carries log(1 / scale)
    assert np.max(np.abs(grad - ours)) < 1e-10 * np.max(np.abs(grad))


@pytest.mark.parametrize("kind", ["sqexponential", "matern52", "matern32"])
def test_gp_ref_against_autograd(kind):
    torch = pytest.importorskip("torch")
    X, y = _data(N=30, seed=1)
    sc = np.array([1.5, 2.5, 0.8])
    mu0 = np.linspace(-0.3, 0.3, len(y))
    ref = _ref(kind, sc, X, y, mu0=mu0)
    lv = torch.tensor(np.log(1.7), dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(np.log(sc), dtype=torch.float64, requires_grad=True)
    ln = torch.tensor(np.log(ref.sigma2), dtype=torch.float64, requires_grad=True)
    Xt = torch.tensor(X)
    d2 = (((Xt[:, None, :] - Xt[None, :, :]) * torch.exp(ls)) ** 2).sum(-1)
    r = torch.sqrt(d2 + 1e-300)
    if kind == "sqexponential":
        b = torch.exp(-0.5 * d2)
    elif kind == "matern52":
        b = (1 + np.sqrt(5) * r + 5.0 / 3.0 * d2) * torch.exp(-np.sqrt(5) * r)
    else:
        b = (1 + np.sqrt(3) * r) * torch.exp(-np.sqrt(3) * r)
    N = len(y)
    S = torch.exp(lv) * b + (JITT + torch.exp(ln)) * torch.eye(N, dtype=torch.float64)
    rr = torch.tensor(y - mu0)
    Lc = torch.linalg.cholesky(S)
    logp = -(rr @ torch.cholesky_solve(rr[:, None], Lc)[:, 0] + 2 * torch.log(torch.diagonal(Lc)).sum() + N * np.log(2 * np.pi)) / 2
    logp.backward()
    assert abs(logp.item() - ref.logp) < 1e-10 * abs(ref.logp)
    gv, gs = ref.hyper_grad()
    assert abs(lv.grad.item() - 1.7 * gv) < 1e-10 * max(1.0, abs(lv.grad.item()))
    assert np.max(np.abs(ls.grad.numpy() - sc * gs)) < 1e-10 * np.max(np.abs(ls.grad.numpy()))
    assert abs(ln.grad.item() - ref.sigma2 * ref.noise_grad()) < 1e-10 * max(1.0, abs(ln.grad.item()))


def test_gp_ref_reference_mode_defects():
    X, y = _data(N=25, seed=2)
    mu0 = 0.4
    a = GPRef(R.Kernel("sqexponential", 2.0, 1.0), X, y, noise=0.05, mu0=mu0, mode="corrected", optimiser=R.Adam(0.01))
    b = GPRef(R.Kernel("sqexponential", 2.0, 1.0), X, y, noise=0.05, mu0=mu0, mode="reference", optimiser=R.Adam(0.01))
    # G3: log p with y in place of y - mu0
    yq = y @ np.linalg.solve(b.Sigma, y)
    assert abs(b.logp + (yq + np.linalg.slogdet(b.Sigma)[1] + len(y) * np.log(2 * np.pi)) / 2) < 1e-10 * abs(b.logp)
    assert abs(a.logp - b.logp) > 1e-3
    # G2: ||alpha||_2 in the noise gradient
    assert abs(b.noise_grad() - (np.linalg.norm(b.alpha) - np.trace(b.Sinv)) / 2) < 1e-12 * abs(b.noise_grad())
    assert abs(a.noise_grad() - (a.alpha @ a.alpha - np.trace(a.Sinv)) / 2) < 1e-12 * abs(a.noise_grad())
    # G1: the kernel never moves in the reference's mode; it does in the corrected one
    a.train(10)
    b.train(10)
    assert b.kernel.sigma2 == 1.0 and b.kernel.scale == 2.0
    assert a.kernel.sigma2 != 1.0 and a.kernel.scale != 2.0


def test_gp_ref_constructor_one_noise_step():
    X, y = _data(N=20, seed=3)
    g = GPRef(R.Kernel("sqexponential", 10.0, 1.0), X, y, noise=1e-2)
    assert g.n_iter == 1 and len(g.sigma2_trace) == 1
    fresh = GPRef(R.Kernel("sqexponential", 10.0, 1.0), X, y, noise=1e-2, construct=False)
    st, d = R.Adam(0.05).apply(R.Adam(0.05).init(np.zeros(1)), np.array([fresh.noise_grad() * 1e-2]))
    assert abs(g.sigma2 - np.exp(np.log(1e-2) + d[0])) < 1e-15


def test_gp_constructor_refusals():
    import agp_amd as AGP

    X, y = _data(N=10)
    k = AGP.SqExponentialKernel()
    with pytest.raises(ValueError, match="same number of samples"):
        AGP.GP(X, y[:-1], k)
    with pytest.raises(NotImplementedError):
        AGP.GP(X, y, k, T=np.float32)
    with pytest.raises(NotImplementedError):
        AGP.GP(X, y, k, optimiser=object())
    assert repr(AGP.Analytic()) == "Analytic Inference"


def test_analytic_only_for_gp():
    """Analytic() is the exact GP's inference: SVGP and VGP keep refusing it as the reference does (SVGP.jl:45-47, VGP.jl:51)"""
    import agp_amd as AGP

    X, y = _data(N=10)
    k = AGP.SqExponentialKernel()
    assert not isinstance(AGP.Analytic(), AGP.AnalyticVI)
    with pytest.raises(TypeError, match="should be of type"):
        AGP.SVGP(k, AGP.GaussianLikelihood(0.1), AGP.Analytic(), X[:4])
    with pytest.raises(TypeError, match="should be of type"):
        AGP.VGP(X, np.sign(y), k, AGP.LogisticLikelihood(), AGP.Analytic())


def test_gp_flag_in_abi():
    from agp_amd import capi

    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    assert re.search(r"AGP_FLAG_EXACT\s*=\s*4", h)
    assert capi.FLAG_EXACT == 4


def test_gp_shim_binding():
    src = open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    assert re.search(r"GP\{[^}]*<:\s*GaussianLikelihood\s*,\s*<:\s*Analytic\s*\}", src)
    assert re.search(r"const AGP_FLAG_EXACT\s*=\s*Int32\(4\)", src)
