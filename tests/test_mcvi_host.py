"""MCIntegrationVI without a GPU: the NumPy restatement tests/_mcvi_ref.py against conditions that do not come from the code under
test (the exact moments of N(0, 1), autograd, the Gauss-Hermite product rule), the margin condition of every GPU parity input, the
constructors of the host mirror, their repr strings and refusals, and the new constants in header and binding."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import _mcvi_cases as CS
import _mcvi_ref as M
import _mcgp_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def AGP():
    import agp_amd

    return agp_amd


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", [M.STREAM_GRAD, M.STREAM_ELBO])
def test_philox_table_moments(stream):
    """10^6 draws: mean, second and fourth moment within 5 standard errors of those of N(0, 1); the standard errors come from the
    exact moments E x^2 = 1, E x^4 = 3, E x^8 = 105 (Var x = 1, Var x^2 = 2, Var x^4 = 96), not from the sample"""
    n = 10 ** 6
    e = M.normals(987654321, 3, stream, n // 8, 8).ravel()
    assert np.all(np.isfinite(e))
    m1, m2, m4 = e.mean(), (e ** 2).mean(), (e ** 4).mean()
    print(f"stream {stream}: mean {m1:.2e} (5 se {5 / math.sqrt(n):.2e}) m2 - 1 {m2 - 1:.2e} ({5 * math.sqrt(2 / n):.2e}) "
          f"m4 - 3 {m4 - 3:.2e} ({5 * math.sqrt(96 / n):.2e})")
    assert abs(m1) < 5 * math.sqrt(1.0 / n)
    assert abs(m2 - 1.0) < 5 * math.sqrt(2.0 / n)
    assert abs(m4 - 3.0) < 5 * math.sqrt(96.0 / n)


def test_table_follows_the_stream_contract():
    """counter (s K + k, t, stream, 0), key = seed, the two uniforms of block 0: the uniforms are those of the scalar generator of
    tests/_mcgp_ref.py; log and cos by the contract's arithmetic agree with the math library to rounding; streams, steps and seeds
    give different tables"""
    K, nMC, seed, t = 3, 50, (5 << 32) + 77, 9
    e = M.normals(seed, t, M.STREAM_GRAD, nMC, K)
    for s, k in ((0, 0), (7, 2), (49, 1)):
        st = G.Stream(seed, t, M.STREAM_GRAD, s * K + k)
        a, b = st.u(), st.u()
        ref = math.sqrt(-2.0 * math.log(a)) * math.cos(6.283185307179586 * b)
        assert e[s, k] == pytest.approx(ref, rel=1e-9, abs=1e-15)  # (2 pi b rounds once in the library form: its cosine moves near a zero)
        assert float(M.mc_log(np.array([a]))[0]) == pytest.approx(math.log(a), rel=4e-16)
    u = np.random.default_rng(0).random(20000)
    assert np.max(np.abs(M.mc_log(u) - np.log(u)) / np.abs(np.log(u))) < 1e-15
    assert np.max(np.abs(M.mc_cos2pi(u) - np.cos(2 * np.pi * u))) < 1e-15
    for other in (M.normals(seed, t, M.STREAM_ELBO, nMC, K), M.normals(seed, t + 1, M.STREAM_GRAD, nMC, K),
                  M.normals(seed + 1, t, M.STREAM_GRAD, nMC, K)):
        assert not np.array_equal(e, other)
    assert np.array_equal(e, M.normals(seed, t, M.STREAM_GRAD, nMC, K))


# ---- 2. the closed forms ------------------------------------------------------------------------------------------------------------
def _torch_ell(torch, link, c, mu, sd, eps):
    f = mu[None, :] + sd[None, :] * eps
    if link == "softmax":
        return (f[:, c] - torch.logsumexp(f, dim=1)).mean()
    return (torch.nn.functional.logsigmoid(f[:, c]) - torch.log(torch.sigmoid(f).sum(dim=1))).mean()


@pytest.mark.parametrize("link", M.LINKS)
@pytest.mark.parametrize("K", [2, 3, 5])
def test_closed_forms_by_autograd(link, K):
    """g = d ell / d mu_k and h = d2 ell / d mu_k2 of the restated ell with eps held fixed, to 1e-10"""
    import torch

    rng = np.random.default_rng(K)
    worst = 0.0
    for trial in range(6):
        mu, var = rng.uniform(-4, 4, K), 10.0 ** rng.uniform(-3, 1, K)
        eps, c = rng.standard_normal((40, K)), int(rng.integers(0, K))
        ell, g, h, _ = M.expectations(link, [c], mu[:, None], var[:, None], eps)
        tm = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
        fn = lambda m: _torch_ell(torch, link, c, m, torch.tensor(np.sqrt(var)), torch.tensor(eps))
        e_t = fn(tm)
        (g_t,) = torch.autograd.grad(e_t, tm)
        H = torch.autograd.functional.hessian(fn, tm)
        worst = max(worst, abs(ell[0] - e_t.item()), np.max(np.abs(g[:, 0] - g_t.numpy())), np.max(np.abs(h[:, 0] - np.diag(H.numpy()))))
    print(f"{link} K={K}: worst difference {worst:.2e}")
    assert worst < 1e-10


@pytest.mark.parametrize("link", M.LINKS)
def test_ell_stays_finite_at_the_corners(link):
    """|mu| = 30 with var = 0: log p of the unlikely class is about -60, where log(softmax(f)) evaluated naively is log(0) = -inf"""
    mu = np.array([[30.0], [-30.0], [-30.0]])
    ell, g, h, _ = M.expectations(link, [1], mu, np.zeros_like(mu), M.normals(1, 1, 2, 10, 3))
    assert np.isfinite(ell[0]) and np.all(np.isfinite(g)) and np.all(np.isfinite(h))
    assert ell[0] == pytest.approx(-60.0 if link == "softmax" else -30.0 - math.log(1.0 + 2 * math.exp(-30.0)) + 0.0, rel=1e-12)
    # and where a class probability approaches one, 1 - s keeps its relative accuracy: g_c = sum of the other probabilities
    ell, g, h, _ = M.expectations("softmax", [0], mu, np.zeros_like(mu), M.normals(1, 1, 2, 10, 3))
    assert g[0, 0] == pytest.approx(2 * math.exp(-60.0), rel=1e-12) and h[0, 0] == pytest.approx(-2 * math.exp(-60.0), rel=1e-12)


# ---- 3. against the product rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", M.LINKS)
@pytest.mark.parametrize("K", [2, 3])
def test_consistency_with_the_gauss_hermite_product_rule(link, K):
    """g and h from 2 10^5 draws against the K-dimensional product rule (20 nodes per axis): within 5 standard errors, the standard
    error from the sample variance of the per-draw terms"""
    rng = np.random.default_rng(10 + K)
    mu, var, c = rng.uniform(-1.5, 1.5, K), rng.uniform(0.2, 1.5, K), 1
    nMC = 200000
    eps = M.normals(4242, 1, M.STREAM_GRAD, nMC, K)
    f = mu[None, :] + np.sqrt(var)[None, :] * eps
    _, Gs, Hs = M.terms(link, c, f)
    x, w = np.polynomial.hermite.hermgauss(20)
    x, w = x * math.sqrt(2.0), w / math.sqrt(math.pi)
    nodes = np.array(list(itertools.product(x, repeat=K)))
    wts = np.prod(np.array(list(itertools.product(w, repeat=K))), axis=1)
    _, Gq, Hq = M.terms(link, c, mu[None, :] + np.sqrt(var)[None, :] * nodes)
    gq, hq = wts @ Gq, wts @ Hq
    for name, S, q in (("g", Gs, gq), ("h", Hs, hq)):
        se = S.std(axis=0, ddof=1) / math.sqrt(nMC)
        z = np.abs(S.mean(axis=0) - q) / se
        print(f"{link} K={K} {name}: |MC - product rule| / se = {np.round(z, 2)}")
        assert np.all(z < 5.0)


# ---- 4. the margin condition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.VGP_CASES) + list(CS.SPARSE_CASES))
def test_margin_condition_on_every_parity_input(name):
    """every matrix whose positive definiteness the backtracking decides has |lambda_min| / lambda_max > 1e-7, so host and device must
    take the same alpha decisions; halvings occur, so the alpha history is exercised; the chain stays finite"""
    tr = CS.trajectory(name) if name in CS.VGP_CASES else CS.sparse_trajectory(name)
    print(f"{name}: smallest margin {tr['margin']:.2e}; (halvings, rejected) per latent {tr['counters']}")
    assert tr["margin"] > 1e-7
    assert sum(c[0] for c in tr["counters"]) > 0 and all(c[1] == 0 for c in tr["counters"])
    assert np.all(np.isfinite(tr["elbo"])) and all(len(a) == len(tr["ref"].lat) for a in tr["alphas"])


def test_elbo_evaluation_is_repeatable_and_moves_with_t():
    """stream 3 at the model's t: two evaluations of an unchanged model agree; the table differs from the gradient draw's"""
    tr = CS.trajectory("softmax-40-nat-descent")
    ref, (X, c) = tr["ref"], CS.data(CS.VGP_CASES["softmax-40-nat-descent"])
    assert ref.elbo(c) == ref.elbo(c) == tr["elbo"][-1] and ref.t == CS.VGP_STEPS


# ---- 5. the host mirror -------------------------------------------------------------------------------------------------------------------
def test_constructors_and_repr(AGP):
    q = AGP.MCIntegrationVI()
    assert (q.eps, q.nMC, q.clipping, q.natural, q.stoch, q.seed) == (1e-5, 1000, math.inf, True, False, 0)
    assert isinstance(q.nvi_optimiser, AGP.Momentum) and q.nvi_optimiser.eta == 0.01        # MCVI.jl:52-58
    assert repr(q) == "Numerical Inference by Monte Carlo Integration"                      # numericalVI.jl:91-96
    s = AGP.MCIntegrationSVI(150)
    assert (s.stoch, s.batchsize, s.nMC, s.clipping, s.natural) == (True, 150, 200, 0.0, True)   # MCVI.jl:83-91
    assert isinstance(s.nvi_optimiser, AGP.Momentum) and s.nvi_optimiser.eta == 0.001
    assert repr(s) == "Stochastic numerical Inference by Monte Carlo Integration"
    s2 = AGP.MCIntegrationSVI(10, nMC=50, optimiser=AGP.ADAM(0.01), natural=False, seed=7, clipping=3.0)
    assert (s2.nMC, s2.seed, s2.natural, s2.clipping) == (50, 7, False, 3.0) and isinstance(s2.nvi_optimiser, AGP.ADAM)
    assert AGP.MCIntegrationVI(seed=5).seed == 5 and AGP.MCIntegrationVI().seed == AGP.MCIntegrationVI().seed
    for bad in (dict(nMC=0), dict(nMC=65537), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            AGP.MCIntegrationVI(**bad)
    with pytest.raises(NotImplementedError, match="Descent, Momentum and ADAM"):
        AGP.MCIntegrationVI(optimiser=AGP.RobbinsMonro())
    l = AGP.SoftMaxLikelihood(4)
    assert repr(l) == "Multiclass Likelihood (4 classes, SoftMax Link )" and l.n_latent == 4     # multiclass.jl:35-37, softmax.jl:24
    l2 = AGP.SoftMaxLikelihood(["a", "b", "c"])
    assert l2.n_class == 3 and l2.class_mapping == ["a", "b", "c"] and l2.lik_desc().kind == 10 and l2.lik_desc().n_class == 3
    with pytest.raises(ValueError):
        AGP.SoftMaxLikelihood(1)
    from agp_amd.likelihoods import likelihood_value

    assert likelihood_value(l2, 2, [0.3, 1.2, -0.5]) == pytest.approx(math.exp(1.2) / (math.exp(0.3) + math.exp(1.2) + math.exp(-0.5)))


def test_models_and_refusals(AGP):
    rng = np.random.default_rng(0)
    X = rng.random((12, 2))
    yc, yb, yr = 1 + np.arange(12) % 3, np.sign(rng.standard_normal(12)), rng.standard_normal(12)
    k = AGP.SqExponentialKernel()
    mc, mcs = AGP.MCIntegrationVI, AGP.MCIntegrationSVI
    for lik in (AGP.SoftMaxLikelihood(3), AGP.LogisticSoftMaxLikelihood(3)):
        m = AGP.VGP(X, yc, k, lik, mc(nMC=20), optimiser=False)
        assert "Numerical Inference by Monte Carlo Integration" in repr(m) and m.n_latent == 3 and m.nvi_alphas == []
        for inf in (mc(nMC=20), mcs(4, nMC=20)):   # the sparse model takes both forms, one kernel for all latents or a list
            assert AGP.SVGP(k, lik, inf, X[:5], optimiser=False).n_latent == 3
            assert len(AGP.SVGP([k, 2.0 * k, k], lik, inf, X[:5], optimiser=False).kernels) == 3
    sm = AGP.SoftMaxLikelihood(3)
    with pytest.raises(NotImplementedError, match="mc"):   # the door that stays shut: its docstring names the entry point
        AGP.NumericalVI("mc")
    assert "MCIntegrationVI" in AGP.NumericalVI.__doc__
    for lik, y in ((AGP.LogisticLikelihood(), yb), (AGP.StudentTLikelihood(3.0), yr), (AGP.LaplaceLikelihood(), yr),
                   (AGP.GaussianLikelihood(), yr), (AGP.BayesianSVM(), yb), (AGP.PoissonLikelihood(2.0), np.abs(yr).astype(int)),
                   (AGP.HeteroscedasticLikelihood(), yr)):
        with pytest.raises(RuntimeError, match="not compatible or implemented"):
            AGP.VGP(X, y, k, lik, mc(), optimiser=False)
        with pytest.raises(RuntimeError, match="not compatible or implemented"):
            AGP.SVGP(k, lik, mc(), X[:5], optimiser=False)
    # the SoftMax likelihood has no augmentation and no quadrature: MC inference only (softmax.jl:22)
    with pytest.raises(RuntimeError, match="not compatible or implemented"):
        AGP.SVGP(k, sm, AGP.AnalyticVI(), X[:5], optimiser=False)
    with pytest.raises(RuntimeError, match="not compatible or implemented"):
        AGP.VGP(X, yc, k, sm, AGP.AnalyticVI(), optimiser=False)
    for lik in (sm, AGP.LogisticSoftMaxLikelihood(3)):    # QuadratureVI with a multi-class likelihood keeps its error
        with pytest.raises(RuntimeError, match="Logistic, StudentT and Laplace"):
            AGP.VGP(X, yc, k, lik, AGP.QuadratureVI(), optimiser=False)
    with pytest.raises(ValueError, match="MCIntegrationSVI"):
        AGP.VGP(X, yc, k, sm, mcs(4), optimiser=False)
    with pytest.raises(NotImplementedError, match="Float64"):
        AGP.VGP(X, yc, k, sm, mc(), optimiser=False, T=np.float32)
    with pytest.raises(NotImplementedError, match="Float64"):
        AGP.SVGP(k, sm, mc(), X[:5], optimiser=False, T=np.float32)
    for opt in (None, True, AGP.ADAM(0.01)):   # the default is refused by name, not silently switched off
        with pytest.raises(NotImplementedError, match="optimiser=False"):
            AGP.VGP(X, yc, k, sm, mc(), optimiser=opt)
        with pytest.raises(NotImplementedError, match="optimiser=False"):
            AGP.SVGP(k, sm, mcs(4), X[:5], optimiser=opt)
    with pytest.raises(NotImplementedError, match="Zoptimiser=False"):
        AGP.SVGP(k, sm, mc(), X[:5], optimiser=False, Zoptimiser=True)
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        AGP.SVGP(k, AGP.SoftMaxLikelihood(65), mc(), X[:5], optimiser=False)
    for inf in (mc(), mcs(4)):
        with pytest.raises(NotImplementedError, match="MOSVGP does not run .*Monte Carlo"):
            AGP.MOSVGP(k, [AGP.LogisticLikelihood()], inf, [X[:5]])
        with pytest.raises(NotImplementedError, match="MOVGP does not run .*Monte Carlo"):
            AGP.MOVGP(X, [yb], k, [AGP.LogisticLikelihood()], inf, 1)
        with pytest.raises(NotImplementedError, match="OnlineSVGP does not run .*Monte Carlo"):
            AGP.OnlineSVGP(k, AGP.LogisticSoftMaxLikelihood(3), inf)
        with pytest.raises(NotImplementedError, match="MCGP does not run .*Monte Carlo"):
            AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), inf)
    with pytest.raises(TypeError):   # exact regression has Analytic() inference built in: there is no inference argument to give
        AGP.GP(X, yr, k, inference=mc())


def test_constants_in_header_and_binding(AGP):
    from agp_amd import capi

    hdr = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    m = re.search(r"AGP_FLAG_MC\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == capi.FLAG_MC == 32
    m = re.search(r"AGP_LIK_SOFTMAX\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == capi.LIK_SOFTMAX == 10
    flags = [int(v) for v in re.findall(r"AGP_FLAG_\w+\s*=\s*(\d+)", hdr)]
    assert len(set(flags)) == len(flags) and all(v & (v - 1) == 0 for v in flags)  # distinct single bits
    for name in ("agp_svgp_mcvi_configure", "agp_mc_normals", "agp_mc_expectations"):
        assert name in capi.SYMBOLS and re.search(r"agp_status\s+" + name + r"\(", hdr)
    assert "MC INTEGRATION" in hdr and "stream 2" in hdr and "stream 3" in hdr
