"""CPU checks of the VGP restatement (tests/_vgp_ref.py), the constructor's refusals and the ABI flag."""
import os
import re

import numpy as np
import pytest

from _liks import labels, oracle_lik
from _vgp_ref import VGPRef
from oracle import agp_ref as R

LIKS = ["logistic", "studentt", "logisticsoftmax", "laplace", "bayesiansvm", "poisson", "negbinomial", "heteroscedastic"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(likname, N=60, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 2))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7
    lik = oracle_lik(R, likname)
    y = R.treat_labels(labels(likname, f, X, rng), lik)
    return X, y, VGPRef(R.Kernel("sqexponential", 2.0, 1.5), lik, X)


def test_one_step_closed_form():
    """Sigma = (K^-1 + 2 diag grad_E_Sigma)^-1 and mu = Sigma grad_E_mu, from the local variables of mu = 0, Sigma = I"""
    X, y, ref = _case("logistic")
    ref.step(y)
    c = np.sqrt(0.0 + 1.0) * np.ones(len(X))  # logistic.jl:39-51 at mean_f = 0, var_f = 1
    theta = np.tanh(c / 2) / (2 * c)
    K = R.Kernel("sqexponential", 2.0, 1.5).matrix(X) + 1e-4 * np.eye(len(X))
    S = np.linalg.inv(np.linalg.inv(K) + np.diag(theta))
    assert np.allclose(ref.Sigma[0], S, rtol=1e-8, atol=1e-10)
    assert np.allclose(ref.mu[0], S @ (y / 2.0), rtol=1e-8, atol=1e-10)


MONOTONE = ["logistic", "studentt", "logisticsoftmax"]


@pytest.mark.parametrize("likname", LIKS)
def test_elbo_trajectory(likname):
    """KAT-6 on the full model.  Logistic, Student-t, LogisticSoftMax: the ELBO never decreases over 30 iterations.  The other five:
    the oracle's ELBO pieces for them are not monotone along CAVI for either model (test_oracle_svgp_is_not_monotone_either pins
    that on the sparse oracle with the same data), so there the trajectory must settle."""
    X, y, ref = _case(likname)
    elbos = []
    for _ in range(30):
        ref.step(y)
        elbos.append(ref.elbo(y))
    assert all(np.isfinite(elbos))
    if likname in MONOTONE:
        assert all(b >= a - 1e-9 * abs(a) for a, b in zip(elbos, elbos[1:])), elbos
    else:
        assert abs(elbos[-1] - elbos[-2]) < 1e-3 * abs(elbos[-1]), elbos


@pytest.mark.parametrize("likname", sorted(set(LIKS) - set(MONOTONE)))
def test_oracle_svgp_is_not_monotone_either(likname):
    """The sparse oracle (R.SVGP, full batch) on the same data falls too at some iteration for these likelihoods: the
    non-monotone VGP trajectory above is a property of the oracle's ELBO terms, not of the VGP restatement."""
    X, y, _ = _case(likname)
    sv = R.SVGP(R.Kernel("sqexponential", 2.0, 1.5), oracle_lik(R, likname), X[:20].copy())
    el = []
    sv.train(X, y, 15, labels_treated=True, callback=lambda M, it, xb, yb: el.append(M.elbo(yb)))
    assert any(b < a - 1e-6 * abs(a) for a, b in zip(el, el[1:])), el


def test_agrees_with_svgp_z_equals_x():
    X, y, ref = _case("logistic", N=50)
    sv = R.SVGP(R.Kernel("sqexponential", 2.0, 1.5), R.LogisticLikelihood(), X.copy())
    sv.train(X, y, 10, labels_treated=True)
    for _ in range(10):
        ref.step(y)
    assert np.max(np.abs(ref.mu[0] - sv.latents[0].mu)) < 1e-2 * np.max(np.abs(ref.mu[0]))


def test_constructor_refusals():
    import agp_amd as AGP

    X = np.random.default_rng(0).random((20, 2))
    y = (X[:, 0] > 0.5).astype(int)
    k = AGP.SqExponentialKernel()
    with pytest.raises(ValueError, match="Gaussian Likelihood"):
        AGP.VGP(X, X[:, 0], k, AGP.GaussianLikelihood(0.1), AGP.AnalyticVI())
    with pytest.raises(ValueError, match="AnalyticVI"):
        AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(5))
    with pytest.raises(NotImplementedError):
        AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), T=np.float32)
    with pytest.raises(TypeError):
        AGP.VGP(X, y, k, AGP.LogisticLikelihood(), "not an inference")
    m = AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=True)
    assert m.k_opt.eta == 0.01  # VGP.jl:63
    assert AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False).k_opt is None
    assert AGP.n_latent(m) == 1 and m.m == 20
    m3 = AGP.VGP(X, y % 3 + 1, k, AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticVI())
    assert AGP.n_latent(m3) == 3


def test_flag_in_header_and_binding():
    from agp_amd import capi

    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    assert re.search(r"AGP_FLAG_FULL = 2", h)
    assert capi.FLAG_FULL == 2


# ---- the generalised hyper-gradient and the prior mean of the restatement ------------------------------------------------------
HKINDS = ["sqexponential", "matern52", "matern32"]


def _trained(likname, kind, scale, N=40, seed=4, mu0=None, steps=3):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 3))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7
    lik = oracle_lik(R, likname)
    y = R.treat_labels(labels(likname, f, X, rng), lik)
    ref = VGPRef(R.Kernel(kind, scale, 1.5), lik, X, mu0=mu0)
    for _ in range(steps):
        ref.step(y)
    return X, y, ref


@pytest.mark.parametrize("kind", HKINDS)
@pytest.mark.parametrize("ard", [False, True])
def test_hyper_grad_matches_autograd(kind, ard):
    from _torch_elbo import neg_kl_hypergrad

    scale = np.array([1.3, 2.2, 0.7]) if ard else 2.0
    X, y, ref = _trained("logistic", kind, scale, mu0=np.linspace(-0.3, 0.4, 40))
    dv, ds = ref.hyper_grad(0)
    av, as_ = neg_kl_hypergrad(kind, X, scale, 1.5, ref.mu[0], ref.mu0[0], ref.Sigma[0])
    assert ds.shape == (3,)
    assert abs(dv - av) < 1e-10 * max(1.0, abs(av)), (dv, av)
    assert np.max(np.abs(ds - as_)) < 1e-10 * max(1.0, np.max(np.abs(as_))), (ds, as_)


def test_hyper_grad_se_scalar_is_the_closed_form():
    """SE with a ScaleTransform: d variance = sum(G o K~) / variance, d s = -s sum(G o K~ o d2), K~ = K - jitt I (the form the
    restatement had before it took any kernel)"""
    X, y, ref = _trained("logistic", "sqexponential", 2.0, mu0=np.full(40, 0.2))
    G = ref.kl_grad_K(0)
    Kb = ref.K - 1e-4 * np.eye(len(X))
    d2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)
    dv, ds = ref.hyper_grad(0)
    assert dv == pytest.approx(float(np.sum(G * Kb) / 1.5), rel=1e-12)
    assert float(np.sum(ds)) == pytest.approx(float(np.sum(G * Kb * (-2.0 * d2))), rel=1e-12)


def test_exponential_hyper_grad_is_refused():
    X, y, ref = _trained("logistic", "exponential", 2.0, steps=1)
    with pytest.raises(ValueError):
        ref.hyper_grad(0)


@pytest.mark.parametrize("likname", ["logistic", "logisticsoftmax"])
def test_step_eta1_carries_the_prior_mean(likname):
    """natural_gradient!(::VarLatent): eta1 = grad_E_mu + K \\ mu0, checked with a direct solve"""
    rng = np.random.default_rng(8)
    mu0 = 0.5 * rng.standard_normal(40)
    X, y, ref = _trained(likname, "matern52", 1.7, mu0=mu0, steps=2)
    ref.step(y)
    g1 = R.grad_E_mu(ref.lik, y, ref.lv)  # the local variables of this step
    K = R.Kernel("matern52", 1.7, 1.5).matrix(X) + 1e-4 * np.eye(len(X))
    for k in range(ref.nl):
        want = g1[k] + np.linalg.solve(K, mu0)
        assert np.max(np.abs(ref.eta1[k] - want)) < 1e-9 * np.max(np.abs(want))
        assert np.max(np.abs(ref.mu0[k] - mu0)) == 0.0


def test_every_latent_owns_its_kernel_and_is_stepped():
    """latentgp.jl:34-36: a deep copy of the kernel per latent; the hyper step moves each with that latent's own gradient"""
    X, y, ref = _trained("logisticsoftmax", "sqexponential", np.array([1.5, 2.5, 1.0]), steps=1)
    assert len({id(k) for k in ref.kernels}) == 3
    grads = [ref.hyper_grad(k) for k in range(3)]
    ref.hyper_step(R.Adam(0.01))
    for k in range(3):
        ker = ref.kernels[k]
        # the first ADAM step moves each log parameter by eta * sign(gradient)
        assert np.log(ker.sigma2 / 1.5) == pytest.approx(0.01 * np.sign(grads[k][0]), rel=1e-6)
        assert np.allclose(np.log(ker.scale / np.array([1.5, 2.5, 1.0])), 0.01 * np.sign(grads[k][1]), rtol=1e-6)
    assert grads[1][0] != grads[0][0] and not np.array_equal(ref.Ks[1], ref.Ks[0])


def test_restatement_keeps_the_se_latent0_trajectory():
    """The hyper trajectory of SE with a scalar scale (what test_vgp_hyper_trajectory compares with) through the per-latent
    restatement equals the one of the single-kernel form: variance, scale and ELBO trace after 8 iterations"""
    X, y, ref = _trained("logistic", "sqexponential", 2.0, N=50, steps=0)
    el = []
    ref.train(y, 8, opt=R.Adam(0.01), callback=lambda r: el.append(r.elbo(y)))
    # the single-kernel form, inline: the same loop with the SE closed form on one shared K
    ker = R.Kernel("sqexponential", 2.0, 1.5)
    o = VGPRef(ker, R.LogisticLikelihood(), X)
    opt, st, el2 = R.Adam(0.01), [None, None], []
    for it in range(8):
        o.step(y)
        el2.append(o.elbo(y))
        if it >= 3 and it + 1 != 8:
            G = o.kl_grad_K(0)
            Kb = o.K - 1e-4 * np.eye(len(X))
            d2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)
            k0 = o.kernels[0]
            gv, gs = float(np.sum(G * Kb) / k0.sigma2), float(np.sum(G * Kb * (-k0.scale * d2)))
            st = [opt.init(np.zeros(1)), opt.init(np.zeros(1))] if st[0] is None else st
            st[0], dv = opt.apply(st[0], np.array([k0.sigma2 * gv]))
            st[1], ds = opt.apply(st[1], np.array([k0.scale * gs]))
            k0.sigma2 = float(np.exp(np.log(k0.sigma2) + dv[0]))
            k0.scale = float(np.exp(np.log(k0.scale) + ds[0]))
            o.refresh_K()
    assert ref.kernel.sigma2 == pytest.approx(o.kernels[0].sigma2, rel=1e-12)
    assert ref.kernel.scale == pytest.approx(o.kernels[0].scale, rel=1e-12)
    assert np.allclose(el, el2, rtol=1e-12, atol=0)
