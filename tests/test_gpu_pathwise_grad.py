"""GPU: input gradients of pathwise samples, paths.grad(X) (include/agp_hip.h agp_pathwise_eval_grad, csrc/agp_pathwise.h,
pathwise.py), against the NumPy restatement tests/_pathwise_grad_ref.py evaluated on the device's OWN tables (paths.tables: omega,
phases, W, V), so that only the evaluation arithmetic differs; bound: the project's parity bound of 1e-8 relative in max norm.
The model recipe is that of tests/test_gpu_pathwise.py: SVGP, Logistic, AnalyticSVI(50), 5 steps on 300 points.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _pathwise_grad_ref as PG
import _pathwise_ref as P
from _pitched import Pitched

pytestmark = pytest.mark.gpu

PARITY = 1e-8
KIND, SCALE, SIGMA2 = "sqexponential", 3.0, 1.5
KINDS = dict(zip(P.KINDS, ("SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel")))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available()
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, L=capi.lib(), torch=torch)


def _kernel(AGP, kind=KIND, scale=SCALE, sigma2=SIGMA2):
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(list(scale))
    return sigma2 * (getattr(AGP, KINDS[kind])() @ tr)


def _data(N, seed=3, D=3, shift=0.0):
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    f = np.sin(2 * X[:, 0]) + 0.5 * X[:, min(1, D - 1)] ** 2 - 0.7
    return rng, X + shift, f


def _build(m, kind=KIND, scale=SCALE, D=3, shift=0.0, idx_stream=False):
    """SVGP, Logistic, AnalyticSVI(50) after 5 steps on 300 points, m inducing points"""
    import agp_amd as AGP

    rng, X, f = _data(300, D=D, shift=shift)
    y = np.sign(f + 0.3 * rng.standard_normal(len(X)))
    Z = rng.standard_normal((m, D)) + shift
    idx = [rng.choice(len(X), 50, replace=False) for _ in range(5)] if idx_stream else None
    model = AGP.SVGP(_kernel(AGP, kind, scale), AGP.LogisticLikelihood(), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
    AGP.train_(model, X, y, 5, idx_stream=idx)
    return model, Z, (X, y)


_svgp = functools.lru_cache(maxsize=None)(lambda m: _build(m))

XT = np.random.default_rng(99).standard_normal((200, 3))


def _xt(n, D, shift=0.0):
    return XT[:n] + shift if D == 3 else np.random.default_rng(99 + D).standard_normal((n, D)) + shift


def _ard(D):
    """ARD scales around sqrt(3 / D): squared scaled distances of a few units in every D, so that the kernel term carries weight"""
    return tuple((0.8 + 0.1 * (d % 5)) * np.sqrt(3.0 / D) for d in range(D))


def _restated(paths, l, kind, scale, Z, X, dtype=np.float64):
    tb = paths.tables(l)
    return PG.grad_tables(kind, scale, SIGMA2, Z, tb["omega"], tb["phase"], tb["W"], tb["V"], X, dtype)


def _check(paths, kind, scale, Z, X, what):
    G = paths.grad(X)
    assert G.shape == (paths.n_samples, len(X), X.shape[1]) and np.all(np.isfinite(G)), what
    err = _rel(G, _restated(paths, 0, kind, scale, Z, X))
    assert err < PARITY, (what, err)
    return err


# ---- closed-form parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_grad_is_the_restatement_on_the_draws_own_tables(env, m):
    AGP = env["AGP"]
    model, Z, _ = _svgp(m)
    errs = []
    for nf in (1, 65, 200):
        for S in (1, 63, 65):
            paths = AGP.sample_paths(model, S, n_features=nf, seed=77, t=nf + S)
            tb = paths.tables(0)
            for nt in (1, 63, 200):
                G = paths.grad(XT[:nt])
                assert G.shape == (S, nt, 3)
                errs.append(_rel(G, PG.grad_tables(KIND, SCALE, SIGMA2, Z, tb["omega"], tb["phase"], tb["W"], tb["V"], XT[:nt])))
                assert errs[-1] < PARITY, (nf, S, nt, errs[-1])
            paths.free()
    print(f"m = {m}: largest relative error of the gradient {max(errs):.2e}")


@pytest.mark.parametrize("D", [1, 3, 33, 64, 65])
@pytest.mark.parametrize("kind", ["matern52", "matern32"])
def test_kernels_and_dimensions(env, kind, D):
    AGP = env["AGP"]
    scale = _ard(D)
    model, Z, _ = _build(65, kind, scale, D)
    paths = AGP.sample_paths(model, 5, n_features=65, seed=13, t=D)
    err = _check(paths, kind, scale, Z, _xt(70, D), (kind, D))
    print(f"{kind}, D = {D}: relative error of the gradient {err:.2e}")


@pytest.mark.parametrize("kind", ["matern52", "matern32"])
def test_points_on_inducing_points(env, kind):
    AGP = env["AGP"]
    scale = _ard(3)
    model, Z, _ = _build(65, kind, scale)
    paths = AGP.sample_paths(model, 5, n_features=65, seed=14, t=0)
    err = _check(paths, kind, scale, Z, Z.copy(), kind)
    print(f"{kind}, X_test = Z: relative error of the gradient {err:.2e}")


@pytest.mark.parametrize("kind,scale", [(KIND, SCALE), ("matern32", _ard(3))])
def test_off_the_origin(env, kind, scale):
    """X, Z and the test points shifted by +100 in every coordinate.  The float64 restatement agrees with its np.longdouble evaluation
    to ~1e-13 on these inputs (asserted below to 1e-11; tests/test_pathwise_grad_host.py has no device to take tables from), so the
    bound tests the kernels, not the reference."""
    AGP = env["AGP"]
    model, Z, _ = _build(65, kind, scale, shift=100.0)
    paths = AGP.sample_paths(model, 5, n_features=65, seed=15, t=0)
    X = _xt(70, 3, shift=100.0)
    X[:5] = Z[:5]
    ref = _restated(paths, 0, kind, scale, Z, X)
    ext = _restated(paths, 0, kind, scale, Z, X, np.longdouble)
    assert np.finfo(np.longdouble).eps < 1e-18 and _rel(ref, ext) < 1e-11, _rel(ref, ext)
    err = _check(paths, kind, scale, Z, X, kind)
    print(f"{kind}, +100: restatement against longdouble {_rel(ref, ext):.2e}, device against the restatement {err:.2e}")


# ---- values, latents, models -----------------------------------------------------------------------------------------------------------
def test_values_are_the_paths_and_the_gradient_is_unchanged(env):
    AGP, torch = env["AGP"], env["torch"]
    model, Z, _ = _svgp(65)
    paths = AGP.sample_paths(model, 5, n_features=65, seed=8, t=1)
    F, G = paths.grad(XT, value=True)
    assert F.shape == (5, 200) and G.shape == (5, 200, 3)
    assert np.array_equal(F, paths(XT)) and np.array_equal(G, paths.grad(XT))
    Fd, Gd = paths.grad(torch.as_tensor(XT, device="cuda"), value=True)  # a device tensor in, device tensors out
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (Fd, Gd))
    assert np.array_equal(Fd.cpu().numpy(), F) and np.array_equal(Gd.cpu().numpy(), G)
    Gt = paths.grad(XT.T.copy(), obsdim=2)
    assert np.array_equal(Gt, G)
    assert paths.grad(np.empty((0, 3))).shape == (5, 0, 3)


def test_logisticsoftmax_one_gradient_per_latent(env):
    AGP = env["AGP"]
    rng, X, f = _data(300)
    y = 1 + (f > -0.9).astype(int) + (f > 0.0).astype(int)
    Z = rng.standard_normal((65, 3))
    model = AGP.SVGP(_kernel(AGP), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    paths = AGP.sample_paths(model, 5, n_features=65, seed=5, t=1)
    F, G = paths.grad(XT[:63], value=True)
    assert G.shape == (3, 5, 63, 3) and np.array_equal(F, paths(XT[:63]))
    errs = [_rel(G[l], _restated(paths, l, KIND, SCALE, model.Zs[l], XT[:63])) for l in range(3)]
    print("largest relative errors of the gradient per latent:", errs)
    assert max(errs) < PARITY and not np.array_equal(G[0], G[1])


def test_vgp_and_exact_gp(env):
    AGP = env["AGP"]
    rng, X, f = _data(130)
    y = np.sign(f + 0.3 * rng.standard_normal(len(X)))
    vgp = AGP.VGP(X, y, _kernel(AGP, "matern52"), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(vgp, 5)
    gp = AGP.GP(X, f + 0.1 * rng.standard_normal(len(X)), _kernel(AGP, "matern32"), noise=0.05, opt_noise=False, optimiser=False)
    AGP.train_(gp, 3)
    for model, kind in ((vgp, "matern52"), (gp, "matern32")):
        paths = AGP.sample_paths(model, 5, n_features=65, seed=21, t=2)
        err = _check(paths, kind, SCALE, X, XT[:63], kind)
        print(f"{type(model).__name__}, N = 130, {kind}: relative error of the gradient {err:.2e}")


# ---- a draw's gradient is a function ---------------------------------------------------------------------------------------------------
def test_chunk_boundary_and_position_independence(env):
    AGP = env["AGP"]
    model, Z, _ = _svgp(63)
    paths = AGP.sample_paths(model, 3, n_features=33, seed=8, t=0)
    n = 4096 + 37
    big = np.random.default_rng(2).standard_normal((n, 3))
    G = paths.grad(big)
    assert G.shape == (3, n, 3) and np.array_equal(G, paths.grad(big))  # two calls, the same bits
    for i in (0, 69, 4095, 4096, n - 1):  # alone, in a block of 70, in the long call: both sides of the chunk edge at 4096
        lo = min(max(i - 35, 0), n - 70)
        assert np.array_equal(paths.grad(big[i:i + 1])[:, 0], G[:, i]), i
        assert np.array_equal(paths.grad(big[lo:lo + 70])[:, i - lo], G[:, i]), i
    err = _rel(G[:, 4000:], _restated(paths, 0, KIND, SCALE, Z, big[4000:]))
    assert err < PARITY, err


def test_pitched_inputs_and_outputs(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    model, Z, _ = _svgp(65)
    S, nt, D = 5, 70, 3
    paths = AGP.sample_paths(model, S, n_features=63, seed=8, t=1)
    F, G = paths.grad(XT[:nt], value=True)
    ldx, ldo, lds, ldg = D + 3, nt + 4, nt + 5, D + 2
    for off in (0, 1):
        for with_f in (True, False):
            xin = Pitched("f64", data=XT[:nt], ld=ldx, off=off, device="cuda")
            fo = Pitched("f64", rows=S, width=nt, ld=ldo, off=off, device="cuda")
            go = Pitched("f64", rows=S * lds, width=D, ld=ldg, off=off, device="cuda")  # [s][i < lds][d < ldg]
            assert L.agp_pathwise_eval_grad(paths._p, C.c_void_p(xin.ptr), ldx, nt, C.c_void_p(fo.ptr) if with_f else None, ldo,
                                            C.c_void_p(go.ptr), lds, ldg) == 0
            torch.cuda.synchronize()
            for buf, name in ((xin, "xt"), (fo, "f_out"), (go, "g_out")):
                buf.check(name)  # every guard element is still the sentinel NaN
            fresh = go.unwritten().reshape(S, lds, D)
            assert not fresh[:, :nt].any() and fresh[:, nt:].all()  # the rows between the samples' blocks are untouched
            assert np.array_equal(go.window().reshape(S, lds, D)[:, :nt], G)
            if with_f:
                assert not fo.unwritten().any() and np.array_equal(fo.window(), F)
            else:
                assert fo.unwritten().all()


def test_sample_mean_agrees_with_predict_f_grad(env):
    """Given the features the paths are i.i.d. over s with mean k* K^-1 mu, so mean_s G estimates dmu of predict_f_grad(cov=False):
    |mean_s G - dmu| / (std_s G / sqrt(S)) < 5 for each of the 60 entries.  S = 2048, 200 features, m = 65, 20 points, seed 31, t = 0.
    The draw's tables are reproducible on the host: the restatement (_pathwise_ref.Draw on the oracle's state after the same five
    minibatches, dmu from the same formula with K^-1 mu in place of V) gives a largest z of 2.65 for this seed (seeds 31 .. 39:
    between 1.59 and 2.87, all below 4)."""
    AGP = env["AGP"]
    model, Z, _ = _build(65, idx_stream=True)
    S, X = 2048, XT[:20]
    paths = AGP.sample_paths(model, S, n_features=200, seed=31, t=0)
    G = paths.grad(X)
    dmu = AGP.predict_f_grad(model, X, cov=False)
    assert G.shape == (S, 20, 3) and dmu.shape == (20, 3)
    z = np.abs(G.mean(axis=0) - dmu) / (G.std(axis=0, ddof=1) / np.sqrt(S))
    print(f"largest z-score of mean_s G against dmu over {z.size} entries: {z.max():.2f}")
    assert np.all(z < 5.0), float(z.max())


def test_snapshot_survives_training_and_the_handle(env):
    AGP, L = env["AGP"], env["L"]
    model, Z, (X, y) = _build(64)
    paths = AGP.sample_paths(model, 4, n_features=65, seed=31, t=2)
    F0, G0 = paths.grad(XT, value=True)
    AGP.train_(model, X, y, 3)
    assert np.array_equal(paths.grad(XT), G0)
    L.agp_svgp_destroy(model._h)
    model._h = None
    F1, G1 = paths.grad(XT, value=True)
    assert np.array_equal(G1, G0) and np.array_equal(F1, F0) and np.array_equal(paths(XT), F0)
    paths.free()
    with pytest.raises(RuntimeError, match="freed"):
        paths.grad(XT)


# ---- refusals and arguments through the ABI ------------------------------------------------------------------------------------------
def _nan(torch, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def test_exponential_kernel_is_refused_by_name(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    from agp_amd.pathwise import GRAD_REFUSAL_EXPONENTIAL

    model, Z, _ = _build(63, "exponential")
    paths = AGP.sample_paths(model, 2, n_features=8, seed=1)
    assert np.all(np.isfinite(paths(XT[:10])))  # the draw itself is fine: only its gradient is refused
    xt = torch.as_tensor(XT[:10], device="cuda").contiguous()
    f, g = _nan(torch, 2, 10), _nan(torch, 2, 10, 3)
    st = L.agp_pathwise_eval_grad(paths._p, C.c_void_p(xt.data_ptr()), 3, 10, C.c_void_p(f.data_ptr()), 10, C.c_void_p(g.data_ptr()), 10, 3)
    msg = L.agp_last_error(model._ctx).decode()
    torch.cuda.synchronize()
    assert st == 5 and "ExponentialKernel" in msg and GRAD_REFUSAL_EXPONENTIAL in msg, (st, msg)
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(g).all())
    with pytest.raises(NotImplementedError, match=GRAD_REFUSAL_EXPONENTIAL):
        paths.grad(XT[:10])


def test_argument_checks(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    model, Z, _ = _svgp(63)
    paths = AGP.sample_paths(model, 2, n_features=8, seed=1)
    xt = torch.as_tensor(XT[:10], device="cuda").contiguous()
    f, g = _nan(torch, 2, 10), _nan(torch, 2, 10, 3)
    px, pf, pg = C.c_void_p(xt.data_ptr()), C.c_void_p(f.data_ptr()), C.c_void_p(g.data_ptr())
    good = dict(xt=px, ldx=3, nt=10, f=pf, ldo=10, g=pg, lds=10, ldg=3)
    cases = {"xt must be given": dict(xt=None), "g_out must be given": dict(g=None), "n_t >= 0": dict(nt=-1), "ldx >= D": dict(ldx=2),
             "lds >= n_t": dict(lds=9), "ldg >= D": dict(ldg=2), "ldo >= n_t": dict(ldo=9)}
    for word, change in cases.items():
        a = {**good, **change}
        st = L.agp_pathwise_eval_grad(paths._p, a["xt"], a["ldx"], a["nt"], a["f"], a["ldo"], a["g"], a["lds"], a["ldg"])
        msg = L.agp_last_error(model._ctx).decode()
        assert st == 1 and "agp_pathwise_eval_grad" in msg and word in msg, (word, st, msg)
    assert L.agp_pathwise_eval_grad(paths._p, px, 3, 10, None, 0, pg, 10, 3) == 0  # ldo is not read without f_out
    torch.cuda.synchronize()
    assert bool(torch.isnan(f).all()) and not bool(torch.isnan(g).any())
    g.fill_(float("nan"))
    assert L.agp_pathwise_eval_grad(paths._p, None, 0, 0, None, 0, None, 0, 0) == 0  # n_t = 0: a successful no-op
    assert L.agp_pathwise_eval_grad(paths._p, px, 3, 0, pf, 10, pg, 10, 3) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(g).all())
