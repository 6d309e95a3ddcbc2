"""CPU tests of pathwise posterior sampling: the restatement (tests/_pathwise_ref.py) against the laws it claims -- the spectral draws
reproduce the four kernels, the rejection-free Gamma has the moments of Gamma(nu, 1), the paths have the stated mean and covariance
given the features -- and the host mirror (pathwise.py): arguments, refusals by name, the bound symbols.  Every statistical bound is
5 standard errors, the standard errors taken from the samples themselves; the seeds are fixed."""
import numpy as np
import pytest

import _pathwise_ref as P

SCALE = (1.5, 0.7, 2.0)  # an ARD transform
SIGMA2 = 1.7


def _within(est, se, truth, what):
    z = np.abs(est - truth) / se
    print(f"{what}: largest z-score {np.max(z):.2f} over {np.size(z)} entries")
    assert np.all(z < 5.0), (what, float(np.max(z)))


@pytest.mark.parametrize("kind", P.KINDS)
def test_spectral_law_reproduces_the_kernel(kind):
    rng = np.random.default_rng(11)
    X = 0.6 * rng.standard_normal((6, 3))
    R, n_features, seed = 400, 256, 20201
    M = np.empty((R, 6, 6))
    for r in range(R):  # independent feature sets: the draw counter t
        om, ph = P.features(kind, 3, n_features, seed, r)
        F = P.phi(X, SCALE, SIGMA2, om, ph)
        M[r] = F @ F.T
    _within(M.mean(axis=0), M.std(axis=0, ddof=1) / np.sqrt(R), P.kernel(kind, SCALE, SIGMA2, X, X), f"E[phi phi'] {kind}")


@pytest.mark.parametrize("kind", ["matern52", "matern32", "exponential"])
def test_rejection_free_gamma_has_the_moments_of_gamma_nu(kind):
    n, nu = 60000, P.NU[kind]
    g = P.gamma_nu(kind, n, 77, 3, latent=1)
    assert np.all(g > 0)
    _within(g.mean(), g.std(ddof=1) / np.sqrt(n), nu, f"mean of G, nu = {nu}")
    c = (g - nu) ** 2
    _within(c.mean(), c.std(ddof=1) / np.sqrt(n), nu, f"variance of G, nu = {nu}")


def _check_moments(F, mean, cov, what):
    S = F.shape[0]
    fm = F.mean(axis=0)
    _within(fm, F.std(axis=0, ddof=1) / np.sqrt(S), mean, what + " mean")
    Fc = F - mean[None, :]  # (the stated mean, so that every product is an unbiased estimate of its covariance entry)
    prod = Fc[:, :, None] * Fc[:, None, :]
    _within(prod.mean(axis=0), prod.std(axis=0, ddof=1) / np.sqrt(S), cov, what + " covariance")


def _posterior(rng, m):
    A = rng.standard_normal((m, m))
    Sigma = 0.3 * A @ A.T / m + 0.2 * np.eye(m)
    return rng.standard_normal(m), Sigma


def test_moments_given_the_features_sparse_form():
    rng = np.random.default_rng(5)
    m, S = 8, 200000
    Z = rng.standard_normal((m, 2))
    Xs = rng.standard_normal((5, 2))
    mu, Sigma = _posterior(rng, m)
    d = P.Draw("matern52", (1.2, 0.8), SIGMA2, Z, S, 16, seed=991, t=2).sparse(mu, -0.5 * np.linalg.inv(Sigma))
    assert np.allclose(np.cov(d.U), Sigma, atol=0.05)  # (u ~ q(u): a coarse sanity check of the square root)
    mean, cov = P.moments_sparse(d, Xs, mu, Sigma)
    _check_moments(d(Xs), mean, cov, "SVGP form")


def test_moments_given_the_features_exact_form():
    rng = np.random.default_rng(6)
    N, S, noise = 8, 200000, 0.3
    X = rng.standard_normal((N, 2))
    Xs = rng.standard_normal((5, 2))
    Sy = P.kernel("sqexponential", 1.3, SIGMA2, X, X) + noise * np.eye(N)
    alpha = np.linalg.solve(Sy, rng.standard_normal(N))
    d = P.Draw("sqexponential", 1.3, SIGMA2, X, S, 16, seed=4242, t=0).exact(alpha, Sy, noise)
    mean, cov = P.moments_exact(d, Xs, alpha, Sy, noise)
    _check_moments(d(Xs), mean, cov, "GP form")


def test_tables_are_functions_of_seed_t_and_latent():
    a = P.features("matern32", 3, 10, 5, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, P.features("matern32", 3, 10, 5, 0)))
    for other in (P.features("matern32", 3, 10, 6, 0), P.features("matern32", 3, 10, 5, 1), P.features("matern32", 3, 10, 5, 0, latent=1)):
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[1], other[1])
    # the SqExponential frequencies are the Normals themselves: the Matern ones are their rescaling, row by row
    z, _ = P.features("sqexponential", 3, 10, 5, 0)
    assert np.allclose(a[0] / z, (a[0] / z)[:, :1])
    assert np.all((a[1] > 0) & (a[1] < 2 * np.pi))
    assert P.table(P.W, 7, 3, 5, 0).shape == (7, 3) and not np.array_equal(P.table(P.W, 7, 3, 5, 0), P.table(P.E, 7, 3, 5, 0))


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
def test_mirror_exports_and_binding_table():
    import agp_amd as AGP
    from agp_amd import capi

    assert callable(AGP.sample_paths) and callable(AGP.pathwise_features) and AGP.PathwiseSamples.__call__
    for name in ("agp_svgp_pathwise_draw", "agp_pathwise_eval", "agp_pathwise_info", "agp_pathwise_get", "agp_pathwise_destroy",
                 "agp_pathwise_features"):
        assert name in capi.SYMBOLS
    assert (capi.PW_OMEGA, capi.PW_PHASE, capi.PW_W, capi.PW_V, capi.PW_E) == (0, 1, 2, 3, 4)
    assert capi.PATHWISE_WS_BYTES == 64 * 1024 * 1024


def test_mirror_argument_limits():
    import agp_amd as AGP
    from agp_amd import pathwise as PW

    Z = np.random.default_rng(0).random((5, 2))
    model = AGP.SVGP(AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z)
    for kw in (dict(n_samples=0), dict(n_samples=65537), dict(n_samples=2, n_features=0), dict(n_samples=2, n_features=65537),
               dict(n_samples=2, t=-1), dict(n_samples=2, t=2 ** 32), dict(n_samples=2, seed=-1), dict(n_samples=2, seed=2 ** 64)):
        with pytest.raises(ValueError):
            AGP.sample_paths(model, **kw)
    PW.check_draw_args(5, 2, 65536, 65535, 2 ** 32 - 1, 2 ** 64 - 1)  # l S = 2^32 - 65536: the largest legal tables
    with pytest.raises(ValueError, match="2\\^32"):
        PW.check_draw_args(5, 2, 65536, 65536, 0)  # l S = 2^32
    with pytest.raises(ValueError, match="2\\^32"):
        PW.check_draw_args(70000, 2, 65536, 8, 0)  # m S
    with pytest.raises(ValueError, match="2\\^32"):
        PW.check_draw_args(5, 70000, 1, 65536, 0)  # l D
    with pytest.raises(TypeError):
        AGP.sample_paths("not a model", 2)


def test_mirror_refusals_by_name():
    import agp_amd as AGP

    rng = np.random.default_rng(0)
    X = rng.random((20, 2))
    y = np.sign(X[:, 0] - 0.5)
    Z = X[:5].copy()
    k = AGP.SqExponentialKernel()
    refused = {
        "Float32": AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z, T=np.float32),
        "multi-output": AGP.MOSVGP(k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticVI(), [Z, Z]),
        "MOVGP": AGP.MOVGP(X, [y, X[:, 1]], k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticVI(), 2),
        "MCGP": AGP.MCGP(X, y, k, AGP.LogisticLikelihood(), AGP.GibbsSampling()),
        "numerical": AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.QuadratureVI(), Z, optimiser=False),
        "follow-up": AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.QuadratureVI(), optimiser=False),
        "latent-sharded": AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(10), Z, latent_slice=(1, 3)),
    }
    for word, model in refused.items():
        with pytest.raises(NotImplementedError, match=word):
            AGP.sample_paths(model, 4)
    # refused before a seed is taken from the model's generator
    assert all(getattr(mdl, "seed", None) is None for mdl in refused.values())
