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
