"""CPU: the restatement of the log predictive density (tests/_lpd_ref.py) against itself at 40 digits, its closed forms and its
Gauss-Hermite rule against the integral, and the host mirror's argument checks, refusals and exports.

Measured error of the 100-node rule in f-space against the integral (test_rule_error_table prints it; absolute error of lpd, worst
over mu in {-1, 0.5, 2}), at sqrt(var_f) / width = 0.1, 1, 10:
    BayesianSVM (width 1, y = 1)               2.9e-04   3.0e-04   6.0e-02     (the kinks of the hinge at f = -+1)
    StudentT nu = 3, sigma = 0.5 (y = 0.3)     4.4e-16   4.2e-08   9.7e-01
    Poisson lambda = 5 (y = 2)                 2.2e-16   4.4e-16   5.0e-02
    NegBinomial r = 3 (y = 2)                  8.9e-16   4.4e-16   1.3e-01
The rule degrades when the predictive spread far exceeds the likelihood's width; these figures are measured, not bounded."""
import inspect
import os
import re

import numpy as np
import pytest

import _lpd_ref as Rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", Rf.GOLDEN))


def _keys(name):
    return [f"lpd{n}" for n in Rf.GRID_NODES] if name in Rf.QUAD else ["lpd"]


# ---- (a) float64 against 40 digits, on the grid of the device test -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Rf.GRID_LIKS))
def test_float64_restatement_against_mpmath(golden, name):
    lik = Rf.GRID_LIKS[name]
    y, mu, var = Rf.grid(name)
    for a, b in ((y, golden[f"{name}/y"]), (mu, golden[f"{name}/mu"]), (var, golden[f"{name}/var"])):
        assert np.array_equal(a, b)  # the fixture belongs to this grid
    for key in _keys(name):
        x, w = Rf.gh_rule(int(key[3:])) if name in Rf.QUAD else (None, None)
        ref = golden[f"{name}/{key}"]
        got = Rf.lpd_np(lik, y, mu, var, x, w)
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
        err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"{name} {key}: worst |float64 - mpmath| / max(1, |ref|) = {err:.2e}")
        assert err <= 1e-13
        # the fixture is the mpmath restatement: every 50th point recomputed
        sel = np.arange(0, Rf.GRID_P, 50)
        again = Rf.lpd_mp(lik, y[sel], mu[..., sel], var[..., sel], x, w)
        assert np.array_equal(again, ref[sel])


def test_the_rows_the_issue_names(golden):
    """mu = -800 y at var = 1e-2 gives about -800 (a direct sum gives -inf); Laplace stays finite at |d| = 50, var = 1e-3 and 30"""
    lg = golden["logistic/lpd100"]
    assert np.all(np.abs(lg[2:4] + 800.0) < 1.0) and np.all(np.abs(lg[4:6]) < 1e-12)  # (log of the weights' sum)
    y, mu, var = Rf.grid("logistic")
    x, w = Rf.gh_rule(100)
    with np.errstate(divide="ignore"):
        direct = np.log(np.sum(w[None, :] * np.exp(Rf.logp_np(("logistic",), y[2:4, None], mu[2:4, None] + 0.1 * x[None, :])), axis=1))
    assert np.all(np.isneginf(direct))
    lp = golden["laplace/lpd"][2:6]
    assert np.all(np.isfinite(lp)) and np.all(lp < -40.0)  # (-|d| / beta = -125 at var = 1e-3; -d^2 / 2 var = -41.7 at var = 30)


# ---- (b) the closed forms and the rule against the integral ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaussian", "laplace"])
def test_closed_forms_against_the_integral(name):
    lik = Rf.GRID_LIKS[name]
    rng = np.random.default_rng(4)
    pts = [(m + rng.standard_normal() * np.sqrt(v + 1.0), m, v) for m, v in zip(rng.uniform(-3, 3, 10), 10.0 ** rng.uniform(-4, 1.5, 10))]
    if name == "laplace":
        pts += [(50.0, 0.0, 30.0), (-50.0, 0.0, 30.0), (5.0, 0.0, 1e-3)]
    kept, worst = 0, 0.0
    for y, m, v in pts:
        ref, ok = Rf.stable_integral(lik, y, m, v)
        if not ok:
            continue
        kept += 1
        got = Rf.lpd_np(lik, np.array([y]), np.array([m]), np.array([v]))[0]
        worst = max(worst, abs(got - ref) / max(1.0, abs(ref)))
    print(f"{name}: {kept} of {len(pts)} inputs with a stable integral, worst error {worst:.2e}")
    assert kept >= len(pts) // 2
    assert worst <= 1e-10


def test_logistic_rule_against_the_integral():
    """mu ~ 3 N(0, 1), var in [1e-6, 31] (the two ends included): bound 1e-4"""
    rng = np.random.default_rng(6)
    n = 40
    mu = 3.0 * rng.standard_normal(n)
    var = 10.0 ** rng.uniform(-6, np.log10(31.0), n)
    var[:4] = (1e-6, 31.0, 31.0, 31.0)
    y = np.sign(rng.standard_normal(n))
    x, w = Rf.gh_rule(100)
    got = Rf.lpd_np(("logistic",), y, mu, var, x, w)
    kept, worst = 0, 0.0
    for i in range(n):
        ref, ok = Rf.stable_integral(("logistic",), y[i], mu[i], var[i])
        if ok:
            kept += 1
            worst = max(worst, abs(got[i] - ref))
    print(f"logistic: {kept} of {n} draws with a stable integral, worst |GH100 - integral| = {worst:.2e}")
    assert kept >= n // 2
    assert worst <= 1e-4


TABLE = [(("bayesiansvm",), 1.0, 1.0), (("studentt", 3.0, 0.5), 0.5, 0.3), (("poisson", 5.0), 1.0, 2.0), (("negbinomial", 3.0), 1.0, 2.0)]


@pytest.mark.parametrize("lik,width,y", TABLE, ids=[t[0][0] for t in TABLE])
def test_rule_error_table(lik, width, y):
    """measured, not bounded: the error of the 100-node rule at sqrt(var) / width = 0.1, 1, 10 (module docstring)"""
    x, w = Rf.gh_rule(100)
    row = []
    for ratio in (0.1, 1.0, 10.0):
        var = (ratio * width) ** 2
        errs = []
        for mu in (-1.0, 0.5, 2.0):
            ref, ok = Rf.stable_integral(lik, y, mu, var)
            assert ok
            got = Rf.lpd_np(lik, np.array([y]), np.array([mu]), np.array([var]), x, w)[0]
            assert np.isfinite(got)
            errs.append(abs(got - ref))
        row.append(max(errs))
    print(f"{lik}: |GH100 - integral| at sqrt(var) / width = 0.1, 1, 10: " + "  ".join(f"{e:.1e}" for e in row))
    assert row[0] <= row[2]  # the rule is at its best where the predictive spread is small against the likelihood's width


# ---- the host mirror ------------------------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    import agp_amd as AGP
    from agp_amd import capi

    p = inspect.signature(AGP.log_predictive_density).parameters
    assert list(p)[:3] == ["model", "X", "y"]
    for name, default in (("pointwise", False), ("n_nodes", 100), ("obsdim", 1)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    q = inspect.signature(AGP.log_predictive_moments).parameters
    assert list(q)[:6] == ["likelihood", "y", "mu", "var", "nodes", "weights"] and q["nodes"].default is None
    assert len(capi.SYMBOLS["agp_svgp_lpd_stream"][1]) == 10 and len(capi.SYMBOLS["agp_log_predictive"][1]) == 12
    hdr = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    assert "LOG PREDICTIVE DENSITY" in hdr
    for sym in ("agp_svgp_lpd_stream", "agp_log_predictive"):
        assert re.search(r"agp_status\s+" + sym + r"\(", hdr)
    for doc in (AGP.log_predictive_density.__doc__, inspect.getmodule(AGP.log_predictive_density).__doc__):
        assert "StudentT" in doc
    assert "as written" in inspect.getmodule(AGP.log_predictive_density).__doc__.lower()


def _refused_models(AGP):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 2))
    yb = np.where(X[:, 0] > 0, 1, -1)
    Z = X[:5].copy()
    k = AGP.SqExponentialKernel()
    svi = lambda: AGP.AnalyticSVI(10)  # noqa: E731
    shard = AGP.SVGP(k, AGP.LogisticLikelihood(), svi(), Z, optimiser=False)
    shard._batch_shard = (0, 2)  # what parallel.HipEngine.set_batch_shard records on the model
    return {
        "Heteroscedastic": AGP.SVGP(k, AGP.HeteroscedasticLikelihood(1.0), svi(), Z, optimiser=False),
        "multi-output": AGP.MOSVGP(k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], svi(), [Z, Z], optimiser=False),
        "MOVGP": AGP.MOVGP(X, [yb, X[:, 1]], k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticVI(), 2,
                           optimiser=False),
        "Gibbs-sampled": AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), AGP.GibbsSampling()),
        "latent-sharded": AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), svi(), Z, optimiser=False, latent_slice=(0, 2)),
        "batch-sharded": shard,
        "not a model": object(),
    }, X, yb


def test_mirror_refuses_before_any_library_call(monkeypatch):
    import agp_amd as AGP
    from agp_amd import capi

    models, X, yb = _refused_models(AGP)

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(capi, "lib", no_library)
    monkeypatch.setattr(capi, "_lib", None)
    for reason, model in models.items():
        with pytest.raises(NotImplementedError, match=reason):
            AGP.log_predictive_density(model, X, yb)
    ok = AGP.SVGP(AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.AnalyticSVI(10), X[:5].copy(), optimiser=False)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_nodes"):
            AGP.log_predictive_density(ok, X, yb, n_nodes=bad)
    # the accepted model classes pass the mirror's own check
    from agp_amd.lpd import lpd_refusal

    accepted = [ok, AGP.VGP(X, yb, AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False),
                AGP.SVGP(AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.QuadratureVI(), X[:5].copy(), optimiser=False),
                AGP.SVGP(AGP.SqExponentialKernel(), AGP.PoissonLikelihood(2.0), AGP.AnalyticSVI(10), X[:5].copy(), optimiser=False)]
    assert [lpd_refusal(m) for m in accepted] == [None] * len(accepted)
    # log_predictive_moments: its argument checks come before the library too
    x, w = Rf.gh_rule(5)
    one = np.ones(3)
    with pytest.raises(NotImplementedError, match="Heteroscedastic"):
        AGP.log_predictive_moments(AGP.HeteroscedasticLikelihood(1.0), one, one, one, x, w)
    with pytest.raises(ValueError, match="needs the Gauss-Hermite"):
        AGP.log_predictive_moments(AGP.LogisticLikelihood(), one, one, one)
    with pytest.raises(ValueError, match="come together"):
        AGP.log_predictive_moments(AGP.LogisticLikelihood(), one, one, one, x)
    with pytest.raises(ValueError, match="one length"):
        AGP.log_predictive_moments(AGP.GaussianLikelihood(0.1), one, one, np.ones(4))
    with pytest.raises(ValueError, match="n_class"):
        AGP.log_predictive_moments(AGP.LogisticSoftMaxLikelihood(3), np.zeros(3, dtype=int), np.ones((2, 3)), np.ones((2, 3)))
