"""CPU tests of the acquisition functions (include/agp_hip.h, "ACQUISITION FUNCTIONS"): the restatement tests/_acq_ref.py against
mpmath and against central differences, the conditioning of every trajectory case the GPU suite runs (on the oracle's objects), and
the host mirror's refusals and argument checks, all of which happen before the device is touched."""
import os
import re

import mpmath
import numpy as np
import pytest

import _acq_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# z grid of the point tests: 901 points in [-37, 8] plus 0 and +-1e-300, at three sigmas; best = xi = 0 so that z = mu / sigma exactly
ZGRID = np.concatenate([np.linspace(-37.0, 8.0, 901), [0.0, 1e-300, -1e-300]])
SIGMAS = (1e-3, 1.0, 1e3)
# UCB on the grid is sigma (z + beta): a beta off the grid's multiples of 0.05, so that no point asks for the relative error of an exact
# zero (nearest z = -0.35: the sum keeps 1 / 20 of its terms)
UCB_BETA = 0.33


def grid_moments():
    """(mu, var) of the grid; the reference is evaluated at exactly these float64 numbers"""
    mu = np.concatenate([ZGRID * s for s in SIGMAS])
    var = np.concatenate([np.full(len(ZGRID), s * s) for s in SIGMAS])
    return mu, var


def mp_point(kind, s, beta, best, xi, mu, var):
    """(alpha, d alpha / d mu, d alpha / d sigma) at 60 digits, as floats; var > 0"""
    with mpmath.workdps(60):
        mu, var, s, beta, best, xi = (mpmath.mpf(float(t)) for t in (mu, var, s, beta, best, xi))
        sg = mpmath.sqrt(var)
        if kind == "ucb":
            return float(s * mu + beta * sg), float(s), float(beta)
        z = (s * (mu - best) - xi) / sg
        P = mpmath.erfc(-z / mpmath.sqrt(2)) / 2
        p = mpmath.exp(-z * z / 2) / mpmath.sqrt(2 * mpmath.pi)
        if kind == "ei":
            return float(sg * (z * P + p)), float(s * P), float(p)
        return float(P), float(s * p / sg), float(-z * p / sg)


def mp_grid(kind, q):
    mu, var = grid_moments()
    return np.array([mp_point(kind, q["s"], q["beta"], q["best"], q["xi"], m, v) for m, v in zip(mu, var)]).T


def assert_close_rel(got, want, bound, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    ok = err <= bound * np.abs(want)
    worst = int(np.argmax(np.where(ok, 0.0, err / np.maximum(np.abs(want), 1e-320))))
    print(f"{what}: worst relative error {np.max(err[want != 0] / np.abs(want[want != 0])) if np.any(want != 0) else 0.0:.3e}")
    assert np.all(ok), (what, worst, got[worst], want[worst])


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_point_function_against_mpmath(kind, minimize):
    q = A.acq(kind, beta=UCB_BETA, minimize=minimize)
    mu, var = grid_moments()
    mu = q["s"] * mu  # (so that z runs over the grid in both directions)
    al, dm, ds, dv = A.point(q, mu, var)
    want = np.array([mp_point(kind, q["s"], q["beta"], 0.0, 0.0, m, v) for m, v in zip(mu, var)]).T
    assert_close_rel(al, want[0], A.PARITY, f"{kind} alpha")
    assert_close_rel(dm, want[1], A.PARITY, f"{kind} d/dmu")
    assert_close_rel(ds, want[2], A.PARITY, f"{kind} d/dsigma")
    assert_close_rel(dv * 2 * np.sqrt(var), want[2], A.PARITY, f"{kind} d/dvar 2 sigma")


def test_point_function_with_incumbent_and_margin():
    rng = np.random.default_rng(3)
    mu, var = rng.normal(0.4, 1.0, 200), rng.uniform(0.01, 2.0, 200)
    for kind in ("ei", "pi"):
        for minimize in (False, True):
            q = A.acq(kind, best=0.7, xi=0.05, minimize=minimize)
            got = A.point(q, mu, var)
            want = np.array([mp_point(kind, q["s"], 0.0, 0.7, 0.05, m, v) for m, v in zip(mu, var)]).T
            for g, w in zip(got[:3], want):
                assert_close_rel(g, w, A.PARITY, kind)


def test_zero_variance_and_nan_rules():
    mu = np.array([-1.0, 0.5, 0.5 + 1e-9, 2.0])
    for var in (0.0, -1e-12):
        v = np.full(4, var)
        for minimize in (False, True):
            s = -1.0 if minimize else 1.0
            al, dm, ds, dv = A.point(A.acq("ucb", beta=2.0, minimize=minimize), mu, v)
            assert np.array_equal(al, s * mu) and np.all(dm == s) and np.all(dv == 0)
            q = A.acq("ei", best=0.5, xi=0.0, minimize=minimize)
            al, dm, ds, dv = A.point(q, mu, v)
            imp = s * (mu - 0.5)
            assert np.array_equal(al, np.maximum(imp, 0.0)) and np.array_equal(dm, np.where(imp > 0, s, 0.0)) and np.all(dv == 0)
            al, dm, ds, dv = A.point(A.acq("pi", best=0.5, minimize=minimize), mu, v)
            assert np.array_equal(al, (imp > 0).astype(float)) and np.all(dm == 0) and np.all(dv == 0)
    for kind in A.KINDS:
        for mu_, var_ in ((np.nan, 1.0), (0.3, np.nan), (np.nan, 0.0), (np.nan, np.nan)):
            out = A.point(A.acq(kind, beta=1.0, best=0.1), [mu_], [var_])
            assert all(np.isnan(t[0]) for t in out), (kind, mu_, var_)


@pytest.mark.parametrize("kind", A.KINDS)
def test_gradient_against_central_differences(kind):
    """the restatement's gradient against central differences of its own alpha, both in long double"""
    name = "m65-logistic-m32-ard"
    parts = A.oracle_parts(name)
    X0, lo, hi, _ = A.inputs(name)
    X = X0[1:12]
    q = A.case_acq(kind, X0, parts, lo, hi)
    _, g, _, _ = A.alpha_grad(q, X, parts, dtype=np.longdouble)
    h = np.longdouble(1e-6)
    fd = np.empty_like(g)
    for d in range(X.shape[1]):
        e = np.zeros(X.shape[1], dtype=np.longdouble)
        e[d] = h
        fp = A.alpha_grad(q, X.astype(np.longdouble) + e, parts, dtype=np.longdouble)[0]
        fm = A.alpha_grad(q, X.astype(np.longdouble) - e, parts, dtype=np.longdouble)[0]
        fd[:, d] = (fp - fm) / (2 * h)
    # truncation h^2 |alpha'''| / 6 ~ 1e-12 scale^3; rounding eps_ld |alpha| / h ~ 1e-13: 1e-8 relative leaves two orders
    assert A.relerr(g, fd) < 1e-8, A.relerr(g, fd)


def test_cases_cover_the_axes():
    sp = [A.spec(n) for n in A.CASES]
    assert {c["m"] for c in sp if c["m"]} >= {1, 63, 64, 65, 130}
    assert {c["D"] for c in sp} >= {1, 3, 4, 5, 17, 33, 64}
    assert {c["R"] for c in A.CASES.values()} >= {1, 63, 64, 65, 4096 + 37}
    assert {t for c in A.CASES.values() for t in c["T"]} == {1, 20}
    kt = {(c["kind"], np.isscalar(c["scale"])) for c in sp}
    assert kt >= {(k, s) for k in ("sqexponential", "matern32", "matern52") for s in (True, False)}
    assert {c["model"] for c in sp} == {"svgp", "vgp", "gp", "quad", "online"}
    assert {A.CASES[n].get("latent", 0) for n in A.CASES} == {0, 2}


@pytest.mark.parametrize("name,kind,T", A.TRAJECTORIES)
def test_conditioning_of_the_trajectory_cases(name, kind, T):
    """float64 against long double over the whole trajectory, on the oracle's objects: what PARITY on the device can rest on"""
    parts = A.oracle_parts(name)
    X0, lo, hi, lr = A.inputs(name)
    q = A.case_acq(kind, X0, parts, lo, hi)
    x64, a64 = A.ascent(q, X0, parts, lo, hi, lr, T)
    xl, al = A.ascent(q, X0, parts, lo, hi, lr, T, dtype=np.longdouble)
    ex = float(np.max(np.abs(x64 - xl)) / np.max(hi - lo))
    ea = A.relerr(a64, al)
    print(f"{name} {kind} T={T}: x {ex:.2e} of the box, alpha {ea:.2e}")
    assert ex <= A.COND_CAP and ea <= A.COND_CAP
    assert np.all(x64 >= lo) and np.all(x64 <= hi) and x64[0, 0] <= hi[0]


# ---- the host mirror: every refusal and argument check before the device is touched ---------------------------------------------------
def _svgp(AGP, kernel=None, D=3, m=5, lik=None, **kw):
    Z = np.random.default_rng(0).standard_normal((m, D))
    return AGP.SVGP(kernel or AGP.SqExponentialKernel(), lik or AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), Z, optimiser=False, **kw)


def _both(AGP, model, match, D=3, exc=NotImplementedError, acq=None):
    acq = acq or AGP.UCB(1.0)
    X = np.zeros((4, D))
    with pytest.raises(exc, match=match):
        AGP.acquisition(model, acq, X)
    with pytest.raises(exc, match=match):
        AGP.maximize_acquisition(model, acq, X, (-1.0, 1.0))


def test_python_refusals():
    import agp_amd as AGP
    from agp_amd.acquisition import acquisition_refusal

    assert acquisition_refusal(_svgp(AGP)) is None and acquisition_refusal(_svgp(AGP, D=64)) is None
    _both(AGP, _svgp(AGP, T=np.float32), "Float32")
    _both(AGP, _svgp(AGP, AGP.ExponentialKernel()), "ExponentialKernel is not differentiable")
    _both(AGP, _svgp(AGP, D=65), "exceeds 64", D=65)
    rng = np.random.default_rng(1)
    Xn = rng.standard_normal((6, 3))
    mo = AGP.MOSVGP(AGP.SqExponentialKernel(), [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticSVI(4),
                    [Xn[:4].copy() for _ in range(2)], Aoptimiser=False, optimiser=False)
    _both(AGP, mo, "multi-output")
    mov = AGP.MOVGP(Xn, [np.sign(Xn[:, 0]), Xn[:, 1]], AGP.SqExponentialKernel(), [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)],
                    AGP.AnalyticVI(), 2, optimiser=False)
    _both(AGP, mov, "multi-output")
    mc = AGP.MCGP(Xn, np.sign(Xn[:, 0]), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    _both(AGP, mc, "MCGP")
    _both(AGP, AGP.SVGP(AGP.SqExponentialKernel(), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticVI(), np.zeros((4, 3)), optimiser=False,
                        latent_slice=(0, 2)), "latent-sharded")
    sh = _svgp(AGP)
    sh._batch_shard = (0, 2)
    _both(AGP, sh, "batch-sharded")
    on = AGP.OnlineSVGP(AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), optimiser=False)
    _both(AGP, on, "not seen a batch")
    _both(AGP, object(), "not a model")


def test_python_argument_checks():
    import agp_amd as AGP

    model, X = _svgp(AGP), np.zeros((4, 3))
    for bad in (lambda: AGP.UCB(-1.0), lambda: AGP.UCB(float("nan")), lambda: AGP.EI(0.0, xi=-0.1), lambda: AGP.PI(0.0, xi=float("inf")),
                lambda: AGP.EI(float("inf"))):
        with pytest.raises(ValueError):
            bad()
    u = AGP.UCB(1.0)
    u.beta = -2.0  # (changed after construction: checked again at the call)
    _both(AGP, model, "beta", exc=ValueError, acq=u)
    with pytest.raises(TypeError, match="UCB"):
        AGP.acquisition(model, "ei", X)
    with pytest.raises(TypeError, match="grad is a bool"):
        AGP.acquisition(model, AGP.UCB(), X, grad=1)
    with pytest.raises(ValueError, match="obsdim"):
        AGP.acquisition(model, AGP.UCB(), X, obsdim=3)
    with pytest.raises(ValueError, match="latent"):
        AGP.acquisition(model, AGP.UCB(), X, latent=1)
    mx = lambda **kw: AGP.maximize_acquisition(model, AGP.UCB(), kw.pop("X0", X), kw.pop("bounds", (-1.0, 1.0)), **kw)
    for kw, match in ((dict(bounds=(1.0, -1.0)), "lo <= hi"), (dict(bounds=(-np.inf, 1.0)), "finite"), (dict(bounds=(0.0,)), "pair"),
                      (dict(steps=-1), "steps"), (dict(steps=65537), "steps"), (dict(lr=0.0), "step sizes"), (dict(beta1=1.0), "beta1"),
                      (dict(beta2=-0.1), "beta2"), (dict(eps=0.0), "eps"), (dict(X0=np.zeros((4, 2))), r"X0 must be"),
                      (dict(X0=np.zeros((0, 3))), "starts"), (dict(latent=3), "latent")):
        with pytest.raises(ValueError, match=match):
            mx(**kw)


def test_best_none_needs_a_model_with_data():
    import agp_amd as AGP

    for acq in (AGP.EI(), AGP.PI()):
        _both(AGP, _svgp(AGP), "best=None", exc=ValueError, acq=acq)
        with pytest.raises(ValueError, match="best must be given"):
            AGP.acquisition_moments(acq, np.zeros(3), np.ones(3))


def test_symbols_are_in_the_header_the_binding_and_the_shim():
    import ctypes as C

    from agp_amd import capi

    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agp_hip.h")).read(), flags=re.S)
    for name, nargs in (("agp_acq_moments", 8), ("agp_svgp_acquisition", 9), ("agp_svgp_acq_maximize", 13)):
        m = re.search(r"agp_status\s+" + name + r"\s*\(([^;]*)\);", h)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(capi.SYMBOLS[name][1]) == nargs
        assert name in open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    assert C.sizeof(capi.AcqDesc) == 32
    assert (capi.VEC_APRED, capi.MAT_APRED) == (11, 12) and "AGP_VEC_APRED = 11" in h and "AGP_MAT_APRED = 12" in h
    assert (capi.ACQ_UCB, capi.ACQ_EI, capi.ACQ_PI) == (0, 1, 2)
