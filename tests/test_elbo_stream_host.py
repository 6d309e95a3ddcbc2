"""CPU tests of the streamed full-data ELBO (agp_svgp_elbo_stream; include/agp_hip.h "STREAMED ELBO"): the declaration, the
binding table, the header's contract, the mirror's refusals and signature, and the oracle restatement the GPU suite compares with."""
import inspect
import os
import re

import numpy as np
import pytest

import _elbo_stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "agp_hip.h")).read()


def test_symbol_is_declared_and_bound_with_nine_arguments():
    from agp_amd import capi

    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"agp_status\s+agp_svgp_elbo_stream\s*\(([^;]*)\)\s*;", src)
    assert decl, "include/agp_hip.h does not declare agp_svgp_elbo_stream"
    assert len(decl.group(1).split(",")) == 9
    res, args = capi.SYMBOLS["agp_svgp_elbo_stream"]
    assert len(args) == 9


def test_header_section_states_the_contract():
    h = _header()
    sec = h[h.index("STREAMED ELBO"):h.index("agp_status agp_svgp_elbo_stream(")]
    flat = " ".join(sec.replace("*", " ").split())
    # once-terms rule
    assert "counted ONCE for the whole stream" in flat and "global point 0" in flat
    assert "log(beta[0])" in flat and "AGP_ELBO_REFERENCE" in flat
    # no-side-effect rule
    assert "No side effects" in flat
    for what in ("the posterior", "local variables of the last step", "validity flags", "look-ahead", "agp_svgp_elbo_terms",
                 "status word"):
        assert what in flat, what
    # refusals and the error codes
    assert "AGP_ERR_UNSUPPORTED" in flat and "before anything is launched" in flat
    for what in ("Poisson", "Heteroscedastic", "opt_noise", "AGP_LIK_MULTIOUTPUT", "AGP_FLAG_FULL", "AGP_FLAG_EXACT",
                 "AGP_FLAG_SAMPLED", "AGP_FLAG_NUMERICAL", "AGP_FLAG_MC", "online", "AGP_FLAG_STALE_K", "latent-sharded",
                 "batch-sharded"):
        assert what in flat, what
    assert "AGP_ERR_NEG_KTILDE" in flat and "FIRST such point" in flat and "stay untouched" in flat
    assert "AGP_ERR_BAD_BATCH" in flat


def _refused_models(AGP, monkeypatch):
    import sys

    # (GP's constructor ends with its one training step, on the device: not what this test is about)
    monkeypatch.setattr(sys.modules[AGP.GP.__module__], "train_", lambda *a, **k: None)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 2))
    yb = np.where(X[:, 0] > 0, 1, -1)
    yc = 1 + (np.arange(20) % 3)
    Z = X[:5].copy()
    k = AGP.SqExponentialKernel()
    svi = lambda: AGP.AnalyticSVI(10)  # noqa: E731
    shard = AGP.SVGP(k, AGP.LogisticLikelihood(), svi(), Z, optimiser=False)
    shard._batch_shard = (0, 2)  # what parallel.HipEngine.set_batch_shard records on the model
    return {
        "Poisson": AGP.SVGP(k, AGP.PoissonLikelihood(2.0), svi(), Z, optimiser=False),
        "Heteroscedastic": AGP.SVGP(k, AGP.HeteroscedasticLikelihood(1.0), svi(), Z, optimiser=False),
        "opt_noise": AGP.SVGP(k, AGP.GaussianLikelihood(0.1, opt_noise=True), svi(), Z, optimiser=False),
        "multi-output": AGP.MOSVGP(k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], svi(), [Z, Z], optimiser=False),
        "full models": AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False),
        "MOVGP": AGP.MOVGP(X, [yb, X[:, 1]], k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticVI(), 2,
                           optimiser=False),
        "exact GP": AGP.GP(X, X[:, 1], k, optimiser=False),
        "Gibbs-sampled": AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), AGP.GibbsSampling()),
        "QuadratureVI": AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.QuadratureVI(), Z, optimiser=False),
        "MCIntegrationVI": AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), AGP.MCIntegrationVI(), Z, optimiser=False),
        "online": AGP.OnlineSVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI()),
        "AGP_FLAG_STALE_K": AGP.SVGP(k, AGP.LogisticLikelihood(), svi(), Z, optimiser=False, reference_compat_stale_K=True),
        "latent-sharded": AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), svi(), Z, optimiser=False, latent_slice=(0, 2)),
        "batch-sharded": shard,
    }, X, yb, yc


def test_mirror_refuses_before_any_library_call(monkeypatch):
    import agp_amd as AGP
    from agp_amd import capi

    models, X, yb, yc = _refused_models(AGP, monkeypatch)

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(capi, "lib", no_library)
    monkeypatch.setattr(capi, "_lib", None)
    for reason, model in models.items():
        with pytest.raises(NotImplementedError, match=reason):
            AGP.elbo_streamed(model, X, yb)
    # ... and through the keyword of ELBO on a sparse model
    with pytest.raises(NotImplementedError, match="Poisson"):
        AGP.ELBO(models["Poisson"], X, np.arange(20) % 4, streamed=True)


def test_signatures():
    import agp_amd as AGP

    sig = inspect.signature(AGP.ELBO)
    assert sig.parameters["streamed"].default is False and sig.parameters["streamed"].kind is inspect.Parameter.KEYWORD_ONLY
    es = inspect.signature(AGP.elbo_streamed).parameters
    assert list(es)[:3] == ["model", "X", "y"]
    for name, default in (("obsdim", 1), ("rho", None), ("idx", None), ("return_terms", False)):
        assert es[name].kind is inspect.Parameter.KEYWORD_ONLY and es[name].default == default


# The restatement (chunks of 4096, predict_f(cov=True) moments, init_local_vars + local_updates, expec_loglikelihood,
# augmented_kl, gaussian_kl) against SVGP.elbo_fresh at N = 8229.  The bound 1e-10 holds for all four (measured: <= 1e-15).
@pytest.mark.parametrize("likname", ["logistic", "gaussian", "studentt", "logisticsoftmax"])
def test_restatement_equals_elbo_fresh(likname):
    from _liks import oracle_lik
    from oracle import agp_ref as R

    X, y, Z, idx = S.data(likname, S.NMAX)
    lik = oracle_lik(R, likname)
    ref = R.SVGP(R.Kernel("sqexponential", S.KSCALE, S.KVAR), lik, Z, stochastic=True, batchsize=S.B)
    ref.train(X, y, S.STEPS, idx_stream=idx)
    yt = R.treat_labels(y, lik)
    want = ref.elbo_fresh(X, yt, 1.0)
    t0, t1, t2 = S.restated_terms(ref, X, yt)
    err = abs((t0 - t1 - t2) - want) / abs(want)
    print(f"{likname}: elbo_fresh {want!r}, restated {t0 - t1 - t2!r}, relative difference {err:.2e}")
    assert err <= 1e-10
    # rho enters as rho t0 - t1 - rho t2
    want = ref.elbo_fresh(X, yt, 2.5)
    assert abs((2.5 * t0 - t1 - 2.5 * t2) - want) / abs(want) <= 1e-10


@pytest.mark.parametrize("name", ["laplace-ref", "logisticsoftmax-ref"])
def test_restatement_counts_the_once_terms_once(name):
    """two chunks (N = 4133): the reference's once-per-evaluation terms enter the restated sum a single time"""
    X, y, yt, Z, idx, ref = S.trained_oracle(name)
    want = ref.elbo_fresh(X, yt, 1.0)
    t0, t1, t2 = S.restated_terms(ref, X, yt)
    assert abs((t0 - t1 - t2) - want) / abs(want) <= 1e-10


def test_reference_var_f_where_the_failure_test_looks():
    """What tests/test_gpu_elbo_stream.py relies on for AGP_ERR_NEG_KTILDE.  In exact arithmetic var_f = K~ + diag(kappa Sigma
    kappa') >= jitter for every posterior agp_svgp_set_state accepts (Sigma = (-2 eta2)^-1 is positive definite or the factorisation
    fails), so no installed state makes it negative: with Sigma = 0 and a point far from Z it is k** + jitter, positive.  A row of x
    that holds a NaN gives moments that are not finite at exactly that point, in the reference too."""
    import copy

    X, y, yt, Z, idx, ref = S.trained_oracle("logistic")
    zero = copy.deepcopy(ref)
    for gp in zero.latents:
        gp.Sigma = np.zeros_like(gp.Sigma)
    mu, var = zero.predict_f(np.full((1, S.D), 50.0), cov=True)
    assert var[0][0] > 0 and abs(var[0][0] - (S.KVAR + zero.jitter)) < 1e-12
    bad = X[:300].copy()
    bad[257, 1] = np.nan
    mu, var = ref.predict_f(bad, cov=True)
    notpos = np.nonzero(~(var[0] > 0))[0]
    assert list(notpos) == [257] and not np.isfinite(mu[0][257])
