"""CPU checks of the MCGP restatement (tests/_mcgp_ref.py: the generator, the samplers against their laws, the chain against the
posterior it must target, the margin condition of the GPU parity inputs) and of the host mirror as far as it runs without a device."""
import math
import os
import re

import numpy as np
import pytest
import scipy.stats as st

import _mcgp_ref as M
from _liks import oracle_lik
from oracle import agp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    """Random123's known answers for Philox4x32-10"""
    f = 0xFFFFFFFF
    assert M.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert M.philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert M.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_uniform_is_open_and_uses_53_bits():
    assert M.u53(0, 0) == 2.0 ** -54 and M.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -54
    s = M.Stream((5 << 32) | 9, 3, 0, 7)
    w = M.philox4x32_10((7, 3, 0, 0), (9, 5))
    assert (s.u(), s.u()) == (M.u53(w[0], w[1]), M.u53(w[2], w[3]))
    w = M.philox4x32_10((7, 3, 0, 1), (9, 5))
    assert s.u() == M.u53(w[0], w[1])


def _pg_draws(n, b, c, seed=1234, t=7):
    z = 0.5 * abs(c)
    r = M.mass_texpon(z)
    return np.array([sum(M.pg1(s, z, r) for _ in range(b)) for s in (M.Stream(seed, t, 0, i) for i in range(n))])


def _mean_in_band(d, m, s2):
    z = (d.mean() - m) / math.sqrt(s2 / len(d))
    print(f"n = {len(d)}  mean {d.mean():.6g}  exact {m:.6g}  z = {z:+.2f}")
    assert abs(z) < 5.0  # 5 sigma: 6e-7 per check


@pytest.mark.parametrize("b,c", [(1, 0.0), (1, 0.5), (1, 2.0), (1, 6.0), (3, 1.0), (7, 0.0)])
def test_polya_gamma_mean(b, c):
    m, s2 = M.pg_moments(b, c)
    _mean_in_band(_pg_draws(20000 if b == 1 else 6000, b, c), m, s2)


@pytest.mark.parametrize("alpha,beta", [(4.5, 2.0), (2.5, 0.7), (3.0, 11.0)])
def test_inverse_gamma_mean_and_shape(alpha, beta):
    n = 20000
    d = np.array([M.inverse_gamma(M.Stream(99, 2, 0, i), alpha, beta) for i in range(n)])
    _mean_in_band(d, beta / (alpha - 1.0), beta ** 2 / ((alpha - 1.0) ** 2 * (alpha - 2.0)))
    D = st.kstest(d, st.invgamma(alpha, scale=beta).cdf).statistic
    print(f"KS D = {D:.4f}  critical {M.ks_critical(1e-6, n):.4f}")
    assert D < M.ks_critical(1e-6, n)


def test_gamma_boost_below_one():
    """alpha < 1 (StudentT with nu < 1): Gamma(alpha + 1) U^(1 / alpha)"""
    n, alpha = 20000, 0.75
    d = np.array([M.gamma_mt(M.Stream(5, 0, 0, i), alpha) for i in range(n)])
    _mean_in_band(d, alpha, alpha)
    assert st.kstest(d, st.gamma(alpha).cdf).statistic < M.ks_critical(1e-6, n)


@pytest.mark.parametrize("c", [0.0, 2.0])
def test_polya_gamma_shape_against_the_gamma_series(c):
    n1, n2 = 40000, 20000
    D = M.ks_two_sample(_pg_draws(n1, 1, c, seed=4321), M.pg1_series(n2, c, np.random.default_rng(8)))
    crit = M.ks_critical(1e-6, n1, n2)
    print(f"KS D = {D:.4f}  critical {crit:.4f}")
    assert D < crit


def test_chain_targets_the_posterior():
    """N = 4, logistic: E[f | y] by self-normalised importance sampling from the prior against the mean of a long restated chain;
    tolerance 5 times the root of the two squared standard errors (batch means / delta method)"""
    rng = np.random.default_rng(0)
    X = rng.random((4, 2))
    y = np.array([1.0, -1.0, 1.0, 1.0])
    ker = R.Kernel("sqexponential", 2.0, 1.5)
    ref = M.MCGPRef(ker, R.LogisticLikelihood(), X, y, seed=31)
    ref.sample(1, discard_initial=200)
    S = ref.sample(6000)
    nb = 30
    bm = S.reshape(nb, -1, 4).mean(axis=1)
    chain_mean, chain_se = S.mean(axis=0), bm.std(axis=0, ddof=1) / math.sqrt(nb)
    n = 400000
    F = rng.standard_normal((n, 4)) @ ref.L.T
    w = np.exp(-np.sum(np.log1p(np.exp(-y * F)), axis=1))
    wn = w / w.sum()
    is_mean = wn @ F
    is_se = np.sqrt(np.sum((wn[:, None] * (F - is_mean)) ** 2, axis=0))
    z = (chain_mean - is_mean) / np.sqrt(chain_se ** 2 + is_se ** 2)
    print("chain", chain_mean, "importance", is_mean, "z", z)
    assert np.all(np.abs(z) < 5.0)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_margin_condition_of_the_parity_chains(name):
    """No accept / reject comparison of a GPU parity input is closer than 1e-7 (relative): device and host arithmetic differ by far
    less, so no decision can flip and stream parity is exact by construction.  A condition on the inputs, not a tolerance."""
    M.MARGINS.clear()
    ref, (n, discard, thinning) = M.case_ref(name)
    ref.sample(n, discard, thinning)
    assert ref.t == 20
    print(f"{len(M.MARGINS)} comparisons, smallest margin {min(M.MARGINS):.2e}")
    assert min(M.MARGINS) >= 1e-7


@pytest.mark.parametrize("likname", ["logistic", "studentt", "negbinomial"])
def test_margin_condition_of_the_local_parity_inputs(likname):
    y, f, seed, t = M.local_inputs(likname)
    M.MARGINS.clear()
    M.sample_local(oracle_lik(R, likname), y, f, seed, t)
    assert min(M.MARGINS) >= 1e-7


def test_kept_sweeps():
    import agp_amd as AGP
    from agp_amd import mcgp

    assert mcgp.kept_sweeps(3, 0, 1) == [1, 2, 3]
    assert mcgp.kept_sweeps(9, 3, 2) == [4 + 2 * k for k in range(9)] and mcgp.kept_sweeps(9, 3, 2)[-1] == 20
    assert mcgp.kept_sweeps(4, 100, 5) == M.kept_sweeps(4, 100, 5) == [101, 106, 111, 116]
    for bad in [(0, 0, 1), (2, -1, 1), (2, 0, 0)]:
        with pytest.raises(ValueError):
            mcgp.kept_sweeps(*bad)
    assert AGP.sample is mcgp.sample


def test_constructor_refusals_and_repr():
    import agp_amd as AGP

    X = np.random.default_rng(0).random((20, 2))
    y = (X[:, 0] > 0.5).astype(int)
    k = AGP.SqExponentialKernel()
    with pytest.raises(TypeError, match="SamplingInference"):
        AGP.MCGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI())
    with pytest.raises(ValueError, match="For a Gaussian Likelihood you should directly use the `GP` model"):
        AGP.MCGP(X, X[:, 0], k, AGP.GaussianLikelihood(0.1), AGP.GibbsSampling())
    for lik in (AGP.LaplaceLikelihood(0.4), AGP.BayesianSVM(), AGP.PoissonLikelihood(2.0), AGP.HeteroscedasticLikelihood(1.0),
                AGP.LogisticSoftMaxLikelihood(3)):
        with pytest.raises(RuntimeError, match="is not compatible or implemented with the Gibbs Sampler"):
            AGP.MCGP(X, y, k, lik, AGP.GibbsSampling())
    with pytest.raises(ValueError, match="r must be an integer"):
        AGP.MCGP(X, y, k, AGP.NegBinomialLikelihood(2.5), AGP.GibbsSampling())
    with pytest.raises(ValueError, match="non-negative integers"):
        AGP.MCGP(X, np.where(np.arange(20) == 3, -1, 2), k, AGP.NegBinomialLikelihood(3.0), AGP.GibbsSampling())
    with pytest.raises(TypeError, match="should be integers"):  # (treat_labels, event.jl:7-13)
        AGP.MCGP(X, np.where(np.arange(20) == 3, 2.5, 2.0), k, AGP.NegBinomialLikelihood(3.0), AGP.GibbsSampling())
    with pytest.raises(NotImplementedError):
        AGP.MCGP(X, y, k, AGP.LogisticLikelihood(), AGP.GibbsSampling(), T=np.float32)
    with pytest.raises(ValueError, match="same number of samples"):
        AGP.MCGP(X, y[:-1], k, AGP.LogisticLikelihood(), AGP.GibbsSampling())
    with pytest.raises(ValueError, match="EmpiricalMean"):
        AGP.MCGP(X, y, k, AGP.LogisticLikelihood(), AGP.GibbsSampling(), mean=np.zeros(3))
    m = AGP.MCGP(X.T, y, k, AGP.LogisticLikelihood(), AGP.GibbsSampling(), obsdim=2)
    assert m.N == 20 and m.D == 2 and AGP.n_latent(m) == 1
    assert repr(m) == "Monte Carlo Gaussian Process with a Bernoulli Likelihood with Logistic Link sampled via Gibbs Sampler "
    assert math.isnan(AGP.objective(m)) and math.isnan(AGP.ELBO(m))
    with pytest.raises(TypeError, match="sample"):
        AGP.train_(m, 3)
    with pytest.raises(RuntimeError, match="no samples yet"):
        m._store_dev()
    assert m.optimiser.eta == 0.01 and m.k_opt is None  # MCGP.jl:42; never used


def test_gibbs_sampling_arguments():
    import agp_amd as AGP

    g = AGP.GibbsSampling()
    assert (g.nBurnin, g.thinning, g.eps, g.n_iter, g.sample_store) == (100, 1, 1e-5, 0, None)
    with pytest.raises(ValueError, match="nBurnin should be positive"):
        AGP.GibbsSampling(nBurnin=-1)
    with pytest.raises(ValueError, match="thinning should be positive"):
        AGP.GibbsSampling(thinning=-2)


def test_flag_and_symbols_in_header_and_binding():
    from agp_amd import capi

    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    assert re.search(r"AGP_FLAG_SAMPLED = 8", h) and capi.FLAG_SAMPLED == 8
    declared = set(re.findall(r"^agp_status (agp_\w+)\(", h, flags=re.M))
    new = {"agp_svgp_gibbs_sample", "agp_svgp_gibbs_counter", "agp_sample_local", "agp_svgp_predict_samples"}
    assert new <= declared
    assert declared <= set(capi.SYMBOLS), declared - set(capi.SYMBOLS)
