"""CPU tests of the multi-start ascent of pathwise samples (paths.maximize, agp_pathwise_maximize): the restatement
tests/_pathwise_max_ref.py against central differences, the conditioning of every case that tests/test_gpu_pathwise_maximize.py
compares on the device, the 1-D maximum, and what the host mirror decides without a device."""
import os

import numpy as np
import pytest

import _pathwise_max_ref as M
import _pathwise_ref as P
from agp_amd.pathwise import check_maximize_args  # the feature under test: without it nothing here means anything

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b, scale):
    return float(np.max(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble))) / scale)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sqexponential", "matern52", "matern32"])
def test_one_restated_step_against_central_differences(kind):
    """m = 65, S = 4 paths with R = 6 random starts each, 130 features, ARD, V a random table.  The gradient that the restated step
    is made of -- each particle's own path -- against central differences (h = 1e-6) of the restated values: bound 1e-8.  And the step
    itself: from m = v = 0 it moves x by lr g / (|g| + eps) to rounding, the values are those at the new x, and descending mirrors it."""
    D, S, R, m, nf = 3, 4, 6, 65, 130
    rng = np.random.default_rng(42)
    Z = rng.standard_normal((m, D))
    d = P.Draw(kind, (0.7, 1.9, 3.1), 1.5, Z, S, nf, seed=4711, t=1)
    tb = dict(omega=d.omega, phase=d.phase, W=d.W, V=rng.standard_normal((m, S)))
    model = (kind, (0.7, 1.9, 3.1), 1.5, Z)
    X0 = rng.uniform(-1, 1, (S, R, D))
    G = M.grads(*model, tb, X0)
    FD = np.empty_like(G)
    for k in range(D):
        e = np.zeros(D)
        e[k] = 1e-6
        FD[:, :, k] = (M.values(*model, tb, X0 + e) - M.values(*model, tb, X0 - e)) / 2e-6
    err = float(np.max(np.abs(FD - G)) / np.max(np.abs(G)))
    print(f"{kind}: max|FD - G| / max|G| = {err:.2e}")
    assert err < 1e-8
    lr = np.array([0.01, 0.02, 0.03])
    X1, F1 = M.ascent(*model, tb, X0, -5.0, 5.0, lr, 1)
    assert np.max(np.abs(X1 - (X0 + lr * G / (np.abs(G) + 1e-8)))) < 1e-15
    assert np.array_equal(F1, M.values(*model, tb, X1))
    Xm, _ = M.ascent(*model, tb, X0, -5.0, 5.0, lr, 1, minimize=True)
    assert np.max(np.abs((Xm - X0) + (X1 - X0))) < 1e-15  # descending mirrors the step


def test_values_restate_the_paths():
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((20, 2))
    for kind in ("sqexponential", "matern52", "matern32"):
        d = P.Draw(kind, 1.3, 1.5, Z, 3, 50, seed=1, t=0)
        d.V = rng.standard_normal((20, 3))
        X = rng.standard_normal((7, 2))
        F = M.value_tables(kind, 1.3, 1.5, Z, d.omega, d.phase, d.W, d.V, X)
        assert np.max(np.abs(F - d(X))) < 1e-13 * np.max(np.abs(F))


def test_best_breaks_ties_low_and_ignores_nan():
    F = np.array([[1.0, 3.0, 3.0, np.nan], [np.nan, np.nan, np.nan, np.nan], [np.nan, -1.0, -2.0, -1.0]])
    X = np.arange(12.0).reshape(3, 4, 1)
    idx, xb, fb = M.best(X, F)
    assert idx.tolist() == [1, 0, 1] and xb[:, 0].tolist() == [1.0, 4.0, 9.0] and fb[0] == 3.0 and np.isnan(fb[1]) and fb[2] == -1.0
    assert M.best(X, F, minimize=True)[0].tolist() == [0, 0, 2]


# ---- the cases of the GPU tests are well conditioned -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_conditioning_cap_and_idx_gap(name):
    """float64 against np.longdouble over the whole trajectory, T = 1 and 20: <= 1e-11 relative to max|hi - lo| for x and to max|f|
    for f, on the case's host surrogate (the device's Omega, phases and W; V from a posterior of the same kind).  And the two best
    values of every path differ by more than 1e-6 max|f|, so the GPU test compares best_idx everywhere."""
    assert np.finfo(np.longdouble).eps < 1e-18
    c = M.CASES[name]
    Z, tb = M.surrogate_tables(name)
    X0, lo, hi, lr = M.case_inputs(name)
    model = (c["kind"], c["scale"], M.SIGMA2, Z)
    for T in M.STEPS:
        X, F = M.ascent(*model, tb, X0, lo, hi, lr, T)
        Xe, Fe = M.ascent(*model, tb, X0, lo, hi, lr, T, dtype=np.longdouble)
        ex, ef = _rel(X, Xe, float(np.max(hi - lo))), _rel(F, Fe, float(np.max(np.abs(Fe))))
        gap = float(np.min(M.top_gap(F)))
        print(f"{name}, T = {T}: float64 against longdouble x {ex:.2e} f {ef:.2e}; smallest gap of the two best {gap:.2e}")
        assert ex <= M.COND_CAP and ef <= M.COND_CAP, (T, ex, ef)
        assert gap > M.GAP, (T, gap)
        assert np.all(X >= lo) and np.all(X <= hi)
    assert np.all(M.ascent(*model, tb, X0, lo, hi, lr, 0)[0][:, 0, 0] == 2.0)  # start 0 lies outside and is clipped onto the face


# ---- the 1-D maximum --------------------------------------------------------------------------------------------------------------------
def test_one_dimensional_maximum_beats_a_grid():
    """An exact GP on 40 points of 2 exp(-x^2) cos 3x, S = 8 paths, 64 uniform starts in [-2, 2], T = 100, lr = 0.005: on every
    path f_best exceeds the largest of 200 grid values by at least 1e-6 max|f| (measured: 7e-6 .. 3e-4)."""
    c = M.ONE_D
    X, y, X0, grid = M.one_d_data()
    d = P.Draw(c["kind"], c["scale"], c["sigma2"], X, c["S"], c["nf"], c["seed"], c["t"])
    Sy = P.kernel(c["kind"], c["scale"], c["sigma2"], X, X) + c["noise"] * np.eye(c["N"])
    d.exact(np.linalg.solve(Sy, y), Sy, c["noise"])
    tb = dict(omega=d.omega, phase=d.phase, W=d.W, V=d.V)
    model = (c["kind"], c["scale"], c["sigma2"], X)
    Xf, F = M.ascent(*model, tb, X0, c["lo"], c["hi"], c["lr"], c["T"])
    _, xb, fb = M.best(Xf, F)
    Fg = M.value_tables(*model, d.omega, d.phase, d.W, d.V, grid)
    margin = (fb - Fg.max(axis=1)) / np.max(np.abs(Fg))
    print("margins over the grid / max|f|:", margin)
    assert np.all(margin >= 1e-6), margin


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------
def test_binding_and_exported_symbol(built):
    import agp_amd as AGP
    from agp_amd import capi

    assert callable(AGP.PathwiseSamples.maximize)
    res, args = capi.SYMBOLS["agp_pathwise_maximize"]
    assert len(args) == 14
    assert capi.lib().agp_pathwise_maximize.argtypes == args  # the library exports it
    with open(os.path.join(ROOT, "include", "agp_hip.h")) as f:
        header = f.read()
    struct = header[header.index("typedef struct {\n  int32_t steps;"):header.index("} agp_pw_ascent_opts;")]
    assert [n for n, _ in capi.PwAscentOpts._fields_] == ["steps", "minimize", "x0_shared", "beta1", "beta2", "eps", "lo_host", "hi_host",
                                                          "lr_host"]
    assert all(n in struct for n, _ in capi.PwAscentOpts._fields_)


GOOD = dict(n_samples=4, D=3, n_latent=1, x0_shape=(5, 3), bounds=(-1.0, 1.0))
BAD = [
    (dict(D=65, x0_shape=(5, 65)), NotImplementedError, "D > 64 is not supported"),
    (dict(latent=1), ValueError, r"latent must lie in \[0, 1\)"),
    (dict(latent=-1), ValueError, "latent must lie in"),
    (dict(x0_shape=(5, 2)), ValueError, r"X0 must be \(R, 3\) for shared starts or \(4, R, 3\) per sample"),
    (dict(x0_shape=(3, 5, 3)), ValueError, "X0 must be"),
    (dict(x0_shape=(5,)), ValueError, "X0 must be"),
    (dict(x0_shape=(0, 3)), ValueError, "the number of starts must be >= 1"),
    (dict(x0_shape=(2 ** 29, 3)), ValueError, r"n_samples \* starts below 2\^31"),
    (dict(bounds=(-1.0,)), ValueError, r"bounds must be a pair \(lo, hi\)"),
    (dict(bounds=([-1.0, -1.0], 1.0)), ValueError, "lo must be a scalar or of length 3"),
    (dict(bounds=(-1.0, [1.0] * 4)), ValueError, "hi must be a scalar or of length 3"),
    (dict(bounds=(-np.inf, 1.0)), ValueError, "the bounds must be finite"),
    (dict(bounds=(-1.0, np.nan)), ValueError, "the bounds must be finite"),
    (dict(bounds=([0.0, 2.0, 0.0], 1.0)), ValueError, "lo <= hi in every dimension"),
    (dict(lr=[0.1, 0.1]), ValueError, "lr must be a scalar or of length 3"),
    (dict(lr=0.0), ValueError, "the step sizes lr must be finite and > 0"),
    (dict(lr=[0.1, np.inf, 0.1]), ValueError, "the step sizes lr must be finite and > 0"),
    (dict(steps=-1), ValueError, r"steps must lie in \[0, 65536\]"),
    (dict(steps=65537), ValueError, "steps must lie in"),
    (dict(beta1=1.0), ValueError, r"beta1 must lie in \[0, 1\)"),
    (dict(beta2=-0.1), ValueError, r"beta2 must lie in \[0, 1\)"),
    (dict(eps=0.0), ValueError, "eps must be finite and > 0"),
    (dict(eps=np.inf), ValueError, "eps must be finite and > 0"),
]


@pytest.mark.parametrize("change,exc,msg", BAD, ids=[f"{i}-{'-'.join(b[0])}" for i, b in enumerate(BAD)])
def test_check_maximize_args_refuses(change, exc, msg):
    with pytest.raises(exc, match=msg):
        check_maximize_args(**{**GOOD, **change})


def test_check_maximize_args_accepts_and_normalises():
    lo, hi, lr, shared, R = check_maximize_args(**GOOD)
    assert shared and R == 5 and lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0] * 3
    assert np.array_equal(lr, 0.02 * (hi - lo))  # the interface default
    lo, hi, lr, shared, R = check_maximize_args(**{**GOOD, "x0_shape": (4, 7, 3), "bounds": ([0.0, 1.0, 2.0], [1.0, 1.0, 4.0]), "lr": 0.5,
                                                   "steps": 0, "beta1": 0.0, "beta2": 0.0})
    assert not shared and R == 7 and lr.tolist() == [0.5] * 3 and lo.tolist() == [0.0, 1.0, 2.0]
    lr = check_maximize_args(**{**GOOD, "bounds": ([0.0, 1.0, 2.0], [1.0, 1.0, 4.0])})[2]
    assert lr.tolist() == [0.02, 1.0, 0.04]  # a pinned dimension: any positive step size, the box holds it


def _hollow(kinds, freed):
    """a PathwiseSamples with no device object behind it: what maximize decides on the host is decided before it needs one"""
    from agp_amd.pathwise import PathwiseSamples

    ps = PathwiseSamples.__new__(PathwiseSamples)
    ps._model, ps._kinds, ps._p = None, tuple(kinds), None if freed else object()
    ps.n_latent, ps.n_samples, ps.D = len(kinds), 2, 3
    return ps


def test_maximize_refuses_on_the_host_before_any_device_call():
    from agp_amd import capi, pathwise

    with pytest.raises(RuntimeError, match="freed"):
        _hollow([capi.K_SQEXP], freed=True).maximize(np.zeros((4, 3)), (-1, 1))
    text = pathwise.GRAD_REFUSAL_EXPONENTIAL
    with open(os.path.join(ROOT, "include", "agp_hip.h")) as f:
        header = f.read()
    doc = header[header.index(" * agp_pathwise_maximize "):header.index(" * agp_pathwise_get ")]
    assert text in " ".join(doc.replace(" *", " ").split()) and "AGP_ERR_UNSUPPORTED" in doc and "D > 64 is not supported" in doc
    ps = _hollow([capi.K_MATERN52, capi.K_EXPONENTIAL], freed=False)  # (no model, no device: refused before either is touched)
    with pytest.raises(NotImplementedError) as ei:
        ps.maximize(np.zeros((4, 3)), (-1, 1), latent=1)
    assert text in str(ei.value)
    with pytest.raises(ValueError, match="latent must lie in"):
        ps.maximize(np.zeros((4, 3)), (-1, 1), latent=2)
    for change, exc, msg in BAD[3:]:
        a = {**GOOD, **change}
        shape = a.pop("x0_shape")
        if np.prod(shape) > 10 ** 6:
            continue
        hollow = _hollow([capi.K_MATERN52], freed=False)
        hollow.n_samples, hollow.D = a.pop("n_samples"), a.pop("D")
        a.pop("n_latent")
        with pytest.raises(exc, match=msg):
            hollow.maximize(np.zeros(shape), a.pop("bounds"), **a)
