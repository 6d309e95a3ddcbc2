"""QuadratureVI without a GPU: the NumPy restatement tests/_nvi_ref.py against conditions that do not come from the code under test
(autograd, a direct ELBO, the Opper-Archambeau fixed point), the margin condition of every GPU parity input, the constructors of the
host mirror, their repr strings and refusals, and the new flag in header and binding."""
import math
import os
import re

import numpy as np
import pytest

import _nvi_cases as CS
import _nvi_ref as Q
from _liks import oracle_lik
from oracle import agp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def AGP():
    import agp_amd

    return agp_amd


def _points(lik, n_pts=40, seed=0):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-4, 4, n_pts)
    var = 10.0 ** rng.uniform(-6, 1, n_pts)
    y = np.sign(rng.standard_normal(n_pts)) if lik.name == "logistic" else mu + rng.standard_normal(n_pts)
    return y, mu, var


@pytest.mark.parametrize("likname", CS.LIKS)
@pytest.mark.parametrize("n", [3, 20, 100])
def test_g_and_h_are_derivatives_of_the_quadrature_sum(likname, n):
    """g = d/d mu_f of sum_j w_j l(mu_f + s x_j), exactly, for any n; likewise h = d2/d mu_f2 for the two smooth likelihoods"""
    import torch

    lik = oracle_lik(R, likname)
    x, w = Q.gh_rule(n)
    y, mu, var = _points(lik)
    ell, g, h, (_, gabs, habs) = Q.expectations(lik, y, mu, var, x, w)
    mt = torch.tensor(mu, requires_grad=True)
    f = mt[:, None] + torch.tensor(np.sqrt(var))[:, None] * torch.tensor(x)[None, :]
    yy = torch.tensor(y)[:, None]
    if likname == "logistic":
        L = -torch.nn.functional.softplus(-yy * f)
    elif likname == "studentt":
        L = -lik.alpha * torch.log1p(((yy - f) / lik.sigma) ** 2)
    else:
        L = -torch.abs(yy - f) / lik.beta
    S = (L * torch.tensor(w)[None, :]).sum()
    (g_t,) = torch.autograd.grad(S, mt, create_graph=True)
    err = np.max(np.abs(g - g_t.detach().numpy()) / gabs)
    print(f"g: worst error relative to sum w |l'| = {err:.2e}")
    assert err < 1e-12
    if likname != "laplace":
        (h_t,) = torch.autograd.grad(g_t.sum(), mt)
        errh = np.max(np.abs(h - h_t.numpy()) / habs)
        print(f"h: worst error relative to sum w |l''| = {errh:.2e}")
        assert errh < 1e-12


def test_laplace_h_is_the_expectation_of_a_delta():
    """E_{N(mu, v)}[-(2 / beta) delta(y - f)] = -(2 / beta) N(y; mu, v): the derivative of g in mu as n grows (g itself converges
    slowly -- sign(y - f) is discontinuous -- so this is a loose, one-sided sanity check of sign and size)"""
    lik = R.LaplaceLikelihood(0.4)
    x, w = Q.gh_rule(100)
    y, mu, var = np.array([0.3]), np.array([0.1]), np.array([0.5])
    h = Q.expectations(lik, y, mu, var, x, w)[2][0]
    exact = -(2.0 / 0.4) * math.exp(-0.5 * 0.2 ** 2 / 0.5) / math.sqrt(2 * math.pi * 0.5)
    assert h == pytest.approx(exact, rel=1e-14)
    from scipy.special import erf

    Eg = lambda m: erf((0.3 - m) / math.sqrt(2 * 0.5)) / 0.4  # E[sign(y - f)] / beta
    fd = (Eg(0.1 + 1e-5) - Eg(0.1 - 1e-5)) / 2e-5
    assert h == pytest.approx(fd, rel=1e-8)


@pytest.mark.parametrize("likname", CS.LIKS)
def test_elbo_matches_a_direct_evaluation(AGP, likname):
    """the restatement's ELBO against scalar loops over the host mirror's point likelihood and a KL from slogdet / solve"""
    from _liks import agp_lik

    case = dict(lik=likname, N=17, natural=True, opt="descent", mean=0.2, kind="sqexponential", scale=2.0)
    X, y, mean, yt, ref = CS.make_ref(case, n=20)
    for _ in range(3):
        ref.step(yt)
    la = agp_lik(AGP, likname)
    tot = 0.0
    for i in range(len(yt)):
        s = math.sqrt(ref.Sigma[i, i])
        tot += sum(wj * AGP.loglikelihood(la, yt[i], ref.mu[i] + s * xj) for xj, wj in zip(ref.x, ref.w))
    d = ref.mu - ref.mu0
    kl = 0.5 * (np.linalg.slogdet(ref.K)[1] - np.linalg.slogdet(ref.Sigma)[1] + np.trace(np.linalg.solve(ref.K, ref.Sigma))
                + d @ np.linalg.solve(ref.K, d) - len(d))
    assert ref.elbo(yt) == pytest.approx(tot - kl, rel=1e-9)


def test_chain_reaches_the_opper_archambeau_fixed_point():
    """mu = K g, Sigma^-1 = K^-1 - Diagonal(h) at convergence -- a condition that does not come from the update rule.  Bound 1e-8,
    the one the device test puts on the same two residuals: the second is formed from inv(K) and inv(Sigma), whose forward error
    is about n cond(K) eps = 40 (2 N / jitter) 1.1e-16 = 3.5e-9 relative to their largest entry (measured here: 4e-14 and 1.5e-9).
    alpha < 1 in the first steps: the backtracking is exercised."""
    ref, y = CS.fixed_point_reference()
    r1, r2 = ref.residuals(y)
    print(f"residuals {r1:.2e} {r2:.2e}; alphas of the first five steps {ref.alphas[:5]}; smallest alpha {min(ref.alphas)}; "
          f"smallest margin {min(ref.margins):.2e}")
    assert r1 < 1e-8 and r2 < 1e-8
    assert min(ref.alphas[:5]) < 1.0 and ref.rejected == 0
    assert min(ref.margins) > 1e-7


@pytest.mark.parametrize("name", list(CS.VGP_CASES))
def test_margin_condition_of_the_parity_inputs(name):
    """no positive-definiteness decision with |lambda_min| / lambda_max below 1e-7, no Laplace node within 1e-7 (|y| + |f| + 1) of
    the kink: then no decision can flip between host and device, and the alpha histories must agree exactly"""
    tr = CS.trajectory(name)
    print(f"{name}: margin {tr['margin']:.2e} node margin {tr['node_margin']} alphas {tr['alphas']}")
    assert tr["margin"] > 1e-7
    if tr["node_margin"] is not None:
        assert tr["node_margin"] > 1e-7
    assert np.all(np.isfinite(tr["elbo"]))


@pytest.mark.parametrize("name", list(CS.SPARSE_CASES))
def test_margin_condition_of_the_sparse_parity_inputs(name):
    tr = CS.sparse_trajectory(name)
    print(f"{name}: margin {tr['margin']:.2e} node margin {tr['node_margin']} alphas {tr['alphas']}")
    assert tr["margin"] > 1e-7 and (tr["node_margin"] is None or tr["node_margin"] > 1e-7)
    assert np.all(np.isfinite(tr["elbo"]))


@pytest.mark.parametrize("name", list(CS.SHORT))
def test_short_horizons_are_short_for_their_stated_reason(name):
    """up to its short horizon the restated chain is well posed (the margin test above, and a perturbation of 1e-14 stays below
    1e-10); by step STEPS it is not, for the reason tests/_nvi_cases.py states"""
    steps, why = CS.SHORT[name]
    s_short = CS.sensitivity(name, steps)
    long = CS.trajectory(name, CS.STEPS)
    print(f"{name}: {steps} steps, sensitivity {s_short:.2e}; by step {CS.STEPS}: {why}, margin {long['margin']:.2e}, "
          f"ELBO {long['elbo'][0]:.4g} -> {long['elbo'][-1]:.4g}")
    assert s_short < 1e-10
    if why == "diverges":
        assert long["elbo"][-1] < -1e4 and long["elbo"][-1] < 100 * long["elbo"][0]
    elif why == "unstable":
        assert CS.sensitivity(name, CS.STEPS) > 1e-9
    else:
        assert long["margin"] < 1e-7


def test_constructors_and_repr(AGP):
    q = AGP.QuadratureVI()
    assert (q.eps, q.nGaussHermite, q.clipping, q.natural, q.stoch) == (1e-5, 100, 0.0, True, False)
    assert isinstance(q.nvi_optimiser, AGP.Momentum) and q.nvi_optimiser.eta == 1e-5
    assert repr(q) == "Numerical Inference by Quadrature"  # numericalVI.jl:91-96
    s = AGP.QuadratureSVI(150, nGaussHermite=30, optimiser=AGP.ADAM(0.01), natural=False)
    assert (s.stoch, s.batchsize, s.nGaussHermite, s.natural) == (True, 150, 30, False)
    assert repr(s) == "Stochastic numerical Inference by Quadrature"
    n = AGP.NumericalVI("quad")
    assert n.nGaussHermite == 20 and n.nvi_optimiser.eta == 1e-3 and repr(n) == "Numerical Inference by Quadrature"
    ns = AGP.NumericalSVI(40, ":quad")
    assert ns.stoch and ns.batchsize == 40 and repr(ns) == "Stochastic numerical Inference by Quadrature"
    x, w = AGP.gauss_hermite_rule(20)
    assert np.sum(w) == pytest.approx(1.0, rel=1e-14) and np.sum(w * x * x) == pytest.approx(1.0, rel=1e-13)
    xr, wr = Q.gh_rule(20)
    assert np.array_equal(x, xr) and np.array_equal(w, wr)


def test_refusals(AGP):
    rng = np.random.default_rng(0)
    X = rng.random((12, 2))
    yb, yr = np.sign(rng.standard_normal(12)), rng.standard_normal(12)
    k = AGP.SqExponentialKernel()
    q = AGP.QuadratureVI
    m = AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), q(), optimiser=False)
    assert "Numerical Inference by Quadrature" in repr(m)
    with pytest.raises(NotImplementedError, match="mc"):
        AGP.NumericalVI("mc")
    with pytest.raises(NotImplementedError, match="mc"):
        AGP.NumericalSVI(10, "mc")
    with pytest.raises(ValueError, match="integration techniques"):
        AGP.NumericalVI("simpson")
    with pytest.raises(NotImplementedError, match="quadratureVI.jl:121-126"):
        q(clipping=1.0)
    with pytest.raises(RuntimeError, match="not compatible"):  # test/likelihood/gaussian.jl:38,59
        AGP.VGP(X, yr, k, AGP.GaussianLikelihood(), q(), optimiser=False)
    for lik, y in ((AGP.BayesianSVM(), yb), (AGP.PoissonLikelihood(2.0), np.abs(yr).astype(int)),
                   (AGP.NegBinomialLikelihood(3.0), np.abs(yr).astype(int)), (AGP.HeteroscedasticLikelihood(), yr),
                   (AGP.LogisticSoftMaxLikelihood(3), 1 + np.arange(12) % 3)):
        with pytest.raises(RuntimeError, match="Logistic, StudentT and Laplace"):
            AGP.VGP(X, y, k, lik, q(), optimiser=False)
    with pytest.raises(NotImplementedError, match="Float64"):
        AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), q(), optimiser=False, T=np.float32)
    with pytest.raises(ValueError, match="QuadratureSVI"):
        AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), AGP.QuadratureSVI(4), optimiser=False)
    for opt in (None, True, AGP.ADAM(0.01)):  # the default is refused as well, not silently switched off
        with pytest.raises(NotImplementedError, match="optimiser=False"):
            AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), q(), optimiser=opt)
    for inf in (q(), AGP.QuadratureSVI(4)):
        s = AGP.SVGP(k, AGP.LogisticLikelihood(), inf, X[:5], optimiser=False)  # the sparse model takes both forms
        assert "Inference by Quadrature" in repr(s)
        for opt in (None, True, AGP.ADAM(0.01)):
            with pytest.raises(NotImplementedError, match="optimiser=False"):
                AGP.SVGP(k, AGP.LogisticLikelihood(), inf, X[:5], optimiser=opt)
        with pytest.raises(NotImplementedError, match="Zoptimiser=False"):
            AGP.SVGP(k, AGP.LogisticLikelihood(), inf, X[:5], optimiser=False, Zoptimiser=True)
        with pytest.raises(RuntimeError, match="not compatible"):
            AGP.SVGP(k, AGP.GaussianLikelihood(), inf, X[:5], optimiser=False)
        with pytest.raises(RuntimeError, match="Logistic, StudentT and Laplace"):
            AGP.SVGP(k, AGP.BayesianSVM(), inf, X[:5], optimiser=False)
        with pytest.raises(NotImplementedError, match="Float64"):
            AGP.SVGP(k, AGP.LogisticLikelihood(), inf, X[:5], optimiser=False, T=np.float32)
        with pytest.raises(NotImplementedError, match="MOSVGP does not run"):
            AGP.MOSVGP(k, [AGP.LogisticLikelihood()], inf, [X[:5]])
        with pytest.raises(NotImplementedError, match="MOVGP does not run"):
            AGP.MOVGP(X, [yb], k, [AGP.LogisticLikelihood()], inf, 1)
        with pytest.raises(NotImplementedError, match="OnlineSVGP does not run"):
            AGP.OnlineSVGP(k, AGP.LogisticLikelihood(), inf)
        with pytest.raises(NotImplementedError, match="MCGP does not run"):
            AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), inf)
    with pytest.raises(NotImplementedError, match="Descent, Momentum and ADAM"):
        q(optimiser=AGP.RobbinsMonro())


def test_flag_in_header_and_binding(AGP):
    from agp_amd import capi

    hdr = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    m = re.search(r"AGP_FLAG_NUMERICAL\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == capi.FLAG_NUMERICAL == 16
    flags = [int(v) for v in re.findall(r"AGP_FLAG_\w+\s*=\s*(\d+)", hdr)]
    assert len(set(flags)) == len(flags) and all(v & (v - 1) == 0 for v in flags)  # distinct single bits
    for name in ("agp_svgp_nvi_configure", "agp_svgp_nvi_step", "agp_svgp_nvi_info", "agp_svgp_nvi_state", "agp_quad_expectations"):
        assert name in capi.SYMBOLS and re.search(r"agp_status\s+" + name + r"\(", hdr)
