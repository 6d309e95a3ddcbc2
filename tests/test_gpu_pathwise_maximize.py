"""GPU: the on-device multi-start ascent of pathwise samples, paths.maximize (include/agp_hip.h agp_pathwise_maximize,
csrc/agp_pathwise.h k_pw_ascent, pathwise.py), against the NumPy restatement tests/_pathwise_max_ref.py evaluated on the device's OWN
tables (paths.tables), so that only the evaluation arithmetic differs; bound: the project's parity bound of 1e-8 relative in max norm.
The cases are those whose conditioning tests/test_pathwise_maximize_host.py checks on a host surrogate; the conditioning cap and the
gap of the two best values are asserted again here on the device's tables before anything is compared.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import _pathwise_max_ref as M
import _pathwise_ref as P
from _pitched import Pitched

pytestmark = pytest.mark.gpu

PARITY = 1e-8
KINDS = dict(zip(P.KINDS, ("SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel")))


def _rel(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (scale if scale is not None else max(np.max(np.abs(b)), 1e-300)))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available()
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, L=capi.lib(), torch=torch)


def _kernel(AGP, kind, scale, sigma2=M.SIGMA2):
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(list(scale))
    return sigma2 * (getattr(AGP, KINDS[kind])() @ tr)


def _target(X):
    return np.sin(2 * X[:, 0]) + 0.5 * X[:, min(1, X.shape[1] - 1)] ** 2 - 0.7


@functools.lru_cache(maxsize=None)
def _model(kind_of_model, m, D, kind, scale):
    """the recipe of tests/test_gpu_pathwise_grad.py: SVGP (or LogisticSoftMax SVGP), Logistic, AnalyticSVI(50), 5 steps on 300
    points, m standard-normal inducing points; VGP and GP on N = m points"""
    import agp_amd as AGP

    rng = np.random.default_rng(500 + m + D)
    Z = rng.standard_normal((m, D))  # _pathwise_max_ref.case_Z: the inducing points of the case's host surrogate
    X = rng.standard_normal((300, D))
    k = _kernel(AGP, kind, scale)
    if kind_of_model == "vgp":
        model = AGP.VGP(Z, np.sign(_target(Z) + 0.3 * rng.standard_normal(m)), k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
        AGP.train_(model, 5)
    elif kind_of_model == "gp":
        model = AGP.GP(Z, _target(Z) + 0.1 * rng.standard_normal(m), k, noise=0.05, opt_noise=False, optimiser=False)
        AGP.train_(model, 3)
    elif kind_of_model == "lsm":
        f = _target(X)
        model = AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
        AGP.train_(model, X, 1 + (f > -0.9).astype(int) + (f > 0.0).astype(int), 5)
    else:
        model = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
        AGP.train_(model, X, np.sign(_target(X) + 0.3 * rng.standard_normal(300)), 5)
    return model, Z


@functools.lru_cache(maxsize=None)
def _case(name):
    """(paths, the restatement's model tuple, the device's tables of the case's latent)"""
    import agp_amd as AGP

    c = M.CASES[name]
    model, Z = _model(c["model"], c["m"], c["D"], c["kind"], c["scale"])
    assert np.array_equal(Z, M.case_Z(name))
    paths = AGP.sample_paths(model, c["S"], n_features=c["nf"], seed=M.SEED, t=M.T_DRAW)
    return paths, (c["kind"], c["scale"], M.SIGMA2, Z), paths.tables(c.get("latent", 0))


def _own_values(paths, X, latent=0):
    """paths(x) taken at each particle's own sample: [S, R]"""
    S, R, D = X.shape
    F = paths(X.reshape(S * R, D))
    F = F[latent] if paths.n_latent > 1 else F
    return np.stack([F[s, s * R:(s + 1) * R] for s in range(S)])


# ---- T = 0 and the trajectories ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_zero_steps_return_the_clipped_starts_and_their_values(env, name):
    c = M.CASES[name]
    paths, model, tb = _case(name)
    X0, lo, hi, lr = M.case_inputs(name)
    xb, fb, idx, X, F = paths.maximize(X0, (lo, hi), steps=0, lr=lr, latent=c.get("latent", 0), full=True)
    full0 = np.broadcast_to(X0, (c["S"],) + X0.shape[-2:])
    assert X.shape == (c["S"], c["R"], c["D"]) and F.shape == (c["S"], c["R"])
    assert np.array_equal(X, np.minimum(np.maximum(full0, lo), hi)) and np.all(X[:, 0, 0] == 2.0)
    err = _rel(F, _own_values(paths, X, c.get("latent", 0)))
    ri, rx, rf = M.best(X, F)
    assert np.array_equal(idx, ri) and np.array_equal(xb, rx) and np.array_equal(fb, rf)
    print(f"{name}, T = 0: f against paths(x) {err:.2e}")
    assert err < PARITY, err


@pytest.mark.parametrize("T", M.STEPS)
@pytest.mark.parametrize("name", list(M.CASES))
def test_trajectory_is_the_restatement_on_the_draws_own_tables(env, name, T):
    c = M.CASES[name]
    paths, model, tb = _case(name)
    X0, lo, hi, lr = M.case_inputs(name)
    rX, rF = M.ascent(*model, tb, X0, lo, hi, lr, T)
    eX, eF = M.ascent(*model, tb, X0, lo, hi, lr, T, dtype=np.longdouble)
    box, fmax = float(np.max(hi - lo)), float(np.max(np.abs(rF)))
    cx, cf = _rel(rX, eX, box), _rel(rF, eF, fmax)
    gap = float(np.min(M.top_gap(rF)))
    assert cx <= M.COND_CAP and cf <= M.COND_CAP and gap > M.GAP, (cx, cf, gap)  # the inputs are well conditioned: a miss is the device's
    xb, fb, idx, X, F = paths.maximize(X0, (lo, hi), steps=T, lr=lr, latent=c.get("latent", 0), full=True)
    ri, rx, rf = M.best(rX, rF)
    errs = dict(X=_rel(X, rX, box), F=_rel(F, rF, fmax), x_best=_rel(xb, rx, box), f_best=_rel(fb, rf, fmax))
    print(f"{name}, T = {T}: device against the restatement {errs}; float64 against longdouble x {cx:.2e} f {cf:.2e}")
    assert max(errs.values()) < PARITY, errs
    assert np.array_equal(idx, ri)
    x2, f2 = paths.maximize(X0, (lo, hi), steps=T, lr=lr, latent=c.get("latent", 0))  # without full: the same best
    assert np.array_equal(x2, xb) and np.array_equal(f2, fb)


def test_device_tensors_in_device_tensors_out(env):
    torch = env["torch"]
    name = "m64-l65-S5-R13-D3-m52-ard"
    paths, model, tb = _case(name)
    X0, lo, hi, lr = M.case_inputs(name)
    ref = paths.maximize(X0, (lo, hi), steps=3, lr=lr, full=True)
    out = paths.maximize(torch.as_tensor(X0, device="cuda"), (lo, hi), steps=3, lr=lr, full=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out) and out[2].dtype == torch.int64
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(ref, out))
    d = paths.maximize(X0, (-2.0, 2.0), steps=3)  # scalar bounds, the default step size 0.02 (hi - lo)
    e = paths.maximize(X0, (lo, hi), steps=3, lr=np.full(3, 0.08))
    assert np.array_equal(d[0], e[0]) and np.array_equal(d[1], e[1])


# ---- the box -----------------------------------------------------------------------------------------------------------------------
def test_box_faces_pins_and_descent(env):
    name = "m64-l65-S5-R13-D3-m52-ard"
    paths, model, tb = _case(name)
    S, R, D = 5, 40, 3
    rng = np.random.default_rng(8)
    X0 = rng.uniform(-3.0, 3.0, (S, R, D))  # many starts outside the box
    lo, hi = np.array([-1.0, 0.3, -1.5]), np.array([1.0, 0.3, 0.5])  # dimension 1 is pinned: lo = hi
    for T in (0, 5):
        X = paths.maximize(X0, (lo, hi), steps=T, lr=0.05, full=True)[3]
        assert np.all(X >= lo) and np.all(X <= hi) and np.all(X[:, :, 1] == 0.3), T
    # particles on the face x_0 = hi_0 whose gradient points outward, and stays so over steps this small: they stay on the face exactly
    Xf = np.minimum(np.maximum(X0, lo), hi)
    Xf[:, :, 0] = hi[0]
    G = M.grads(*model, tb, Xf)
    out = G[:, :, 0] > 0.2 * np.max(np.abs(G))
    assert out.sum() >= 5
    X = paths.maximize(Xf, (lo, hi), steps=5, lr=1e-3, full=True)[3]
    rX = M.ascent(*model, tb, Xf, lo, hi, 1e-3, 5)[0]
    assert np.all(rX[:, :, 0][out] == hi[0]) and np.all(X[:, :, 0][out] == hi[0])
    # minimize = maximising the negated draw
    neg = dict(tb, W=-tb["W"], V=-tb["V"])
    rX, rF = M.ascent(*model, neg, X0, -2.0, 2.0, 0.03, 20)
    xb, fb, idx, X, F = paths.maximize(X0, (-2.0, 2.0), steps=20, lr=0.03, minimize=True, full=True)
    ri, rx, rf = M.best(rX, rF)
    errs = (_rel(X, rX, 4.0), _rel(F, -rF), _rel(xb, rx, 4.0), _rel(fb, -rf))
    print("minimize against maximising the negated tables:", errs)
    assert max(errs) < PARITY and np.array_equal(F.argmin(axis=1), idx) and np.all(fb == F.min(axis=1))


# ---- a particle is a function of its own inputs --------------------------------------------------------------------------------------
def test_bitwise_independence_of_position_tile_mates_sharing_and_repeats(env):
    AGP = env["AGP"]
    model, Z = _model("svgp", 64, 3, "sqexponential", 3.0)
    rng = np.random.default_rng(2)
    kw = dict(steps=7, lr=0.03, full=True)
    one = AGP.sample_paths(model, 1, n_features=33, seed=8, t=0)
    n = 4096 + 37
    big = rng.uniform(-2.5, 2.5, (n, 3))
    _, _, _, X, F = one.maximize(big, (-2.0, 2.0), **kw)
    again = one.maximize(big, (-2.0, 2.0), **kw)
    assert np.array_equal(again[3], X) and np.array_equal(again[4], F)  # a second call
    for i in (0, 15, 16, 63, 64, 4095, 4096, n - 1):
        alone = one.maximize(big[i:i + 1], (-2.0, 2.0), **kw)
        assert np.array_equal(alone[3][0, 0], X[0, i]) and np.array_equal(alone[4][0, 0], F[0, i]), i
        for at, block in ((0, np.vstack([big[i:i + 1], big[100:164]])), (64, np.vstack([big[100:164], big[i:i + 1]]))):  # first, last of 65
            o = one.maximize(block, (-2.0, 2.0), **kw)
            assert np.array_equal(o[3][0, at], X[0, i]) and np.array_equal(o[4][0, at], F[0, i]), i
    five = AGP.sample_paths(model, 5, n_features=33, seed=8, t=0)
    starts = big[:13]
    sh = five.maximize(starts, (-2.0, 2.0), **kw)
    rep = five.maximize(np.broadcast_to(starts, (5, 13, 3)).copy(), (-2.0, 2.0), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(sh, rep))  # x0_shared against the same starts replicated per sample
    few = five.maximize(starts[3:10], (-2.0, 2.0), **kw)  # other numbers in the call, other tile mates
    assert np.array_equal(few[3], sh[3][:, 3:10]) and np.array_equal(few[4], sh[4][:, 3:10])


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def _opts(capi, T, lo, hi, lr, shared=0, minimize=0, beta1=0.9, beta2=0.999, eps=1e-8):
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, lr)]
    ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in keep]
    return capi.PwAscentOpts(T, minimize, shared, beta1, beta2, eps, *ptr), keep


def test_pitched_inputs_and_outputs_and_null_outputs(env):
    L, torch, capi = env["L"], env["torch"], env["capi"]
    name = "m64-l65-S5-R13-D3-m52-ard"
    paths, model, tb = _case(name)
    S, R, D, T = 5, 13, 3, 4
    X0 = np.random.default_rng(4).uniform(-2.5, 2.5, (S, R, D))
    lo, hi, lr = np.full(D, -2.0), np.full(D, 2.0), np.full(D, 0.03)
    xb, fb, idx, X, F = paths.maximize(X0, (lo, hi), steps=T, lr=lr, full=True)
    opts, keep = _opts(capi, T, lo, hi, lr)
    ldx0, ldxo, ldf, ldb = D + 3, D + 2, R + 4, D + 1
    for off in (0, 1):
        for given in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 0, 1, 0, 1)):
            xin = Pitched("f64", data=X0.reshape(S * R, D), ld=ldx0, off=off, device="cuda")
            xo = Pitched("f64", rows=S * R, width=D, ld=ldxo, off=off, device="cuda")
            fo = Pitched("f64", rows=S, width=R, ld=ldf, off=off, device="cuda")
            bx = Pitched("f64", rows=S, width=D, ld=ldb, off=off, device="cuda")
            bf = Pitched("f64", rows=1, width=S, off=off, device="cuda")
            bi = Pitched("i64", rows=1, width=S, off=off, device="cuda")
            bufs = (xo, fo, bx, bf, bi)
            p = [C.c_void_p(b.ptr) if g else None for b, g in zip(bufs, given)]
            assert L.agp_pathwise_maximize(paths._p, 0, C.c_void_p(xin.ptr), ldx0, R, C.byref(opts), p[0], ldxo, p[1], ldf, p[2], ldb, p[3],
                                           p[4]) == 0
            torch.cuda.synchronize()
            for buf, what in zip((xin,) + bufs, ("x0", "x_out", "f_out", "best_x", "best_f", "best_idx")):
                buf.check(what)  # every guard element and all padding between the rows is still the sentinel
            want = (X.reshape(S * R, D), F, xb, fb[None, :], idx[None, :])
            for buf, g, w in zip(bufs, given, want):
                if g:
                    assert not buf.unwritten().any() and np.array_equal(buf.window(), w), (off, given)
                else:
                    assert buf.unwritten().all(), (off, given)


# ---- snapshot ----------------------------------------------------------------------------------------------------------------------
def test_snapshot_survives_training_set_kernel_and_the_handle(env):
    AGP, L = env["AGP"], env["L"]
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 3))
    y = np.sign(_target(X) + 0.3 * rng.standard_normal(300))
    model = AGP.SVGP(_kernel(AGP, "sqexponential", 3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(50), rng.standard_normal((64, 3)),
                     optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    paths = AGP.sample_paths(model, 4, n_features=65, seed=31, t=2)
    X0 = rng.uniform(-2, 2, (9, 3))
    ref = paths.maximize(X0, (-2.0, 2.0), steps=6, full=True)
    AGP.train_(model, X, y, 3)
    assert all(np.array_equal(a, b) for a, b in zip(ref, paths.maximize(X0, (-2.0, 2.0), steps=6, full=True)))
    kd, keep = _kernel(AGP, "matern32", 0.7, 2.0).desc(3)
    model._chk(L.agp_svgp_set_kernel(model._h, 0, C.byref(kd)))
    model._chk(L.agp_svgp_refresh_K(model._h))
    assert all(np.array_equal(a, b) for a, b in zip(ref, paths.maximize(X0, (-2.0, 2.0), steps=6, full=True)))
    L.agp_svgp_destroy(model._h)
    model._h = None
    assert all(np.array_equal(a, b) for a, b in zip(ref, paths.maximize(X0, (-2.0, 2.0), steps=6, full=True)))
    paths.free()
    with pytest.raises(RuntimeError, match="freed"):
        paths.maximize(X0, (-2.0, 2.0))


# ---- the 1-D maximum ---------------------------------------------------------------------------------------------------------------
def test_one_dimensional_maximum_beats_a_grid(env):
    """the case of tests/test_pathwise_maximize_host.py on the device: f_best exceeds the path's largest value on a 200-point grid by at
    least 1e-6 max|f| on every one of the 8 paths (the grid values are the device's own paths(grid))"""
    AGP = env["AGP"]
    c = M.ONE_D
    X, y, X0, grid = M.one_d_data()
    gp = AGP.GP(X, y, _kernel(AGP, c["kind"], c["scale"], c["sigma2"]), noise=c["noise"], opt_noise=False, optimiser=False)
    AGP.train_(gp, 3)
    paths = AGP.sample_paths(gp, c["S"], n_features=c["nf"], seed=c["seed"], t=c["t"])
    xb, fb = paths.maximize(X0, (c["lo"], c["hi"]), steps=c["T"], lr=c["lr"])
    Fg = paths(grid)
    margin = (fb - Fg.max(axis=1)) / np.max(np.abs(Fg))
    print("margins over the grid / max|f|:", margin)
    assert xb.shape == (8, 1) and np.all(margin >= 1e-6), margin


# ---- asynchronous --------------------------------------------------------------------------------------------------------------------
def test_the_call_returns_while_the_device_still_works(env):
    """S = R = 64, T = 200: an event recorded behind the call is not ready when the call has returned"""
    AGP, L, torch, capi = env["AGP"], env["L"], env["torch"], env["capi"]
    model, Z = _model("svgp", 130, 33, "sqexponential", M.ard(33))
    S = R = 64
    D = 33
    paths = AGP.sample_paths(model, S, n_features=200, seed=3, t=0)
    x0 = torch.as_tensor(np.random.default_rng(1).uniform(-2, 2, (S, R, D)), device="cuda").contiguous()
    xo = torch.empty(S, R, D, dtype=torch.float64, device="cuda")
    bf = torch.empty(S, dtype=torch.float64, device="cuda")
    opts, keep = _opts(capi, 200, np.full(D, -2.0), np.full(D, 2.0), np.full(D, 0.01))
    args = (paths._p, 0, C.c_void_p(x0.data_ptr()), D, R, C.byref(opts), C.c_void_p(xo.data_ptr()), D, None, 0, None, 0,
            C.c_void_p(bf.data_ptr()), None)
    assert L.agp_pathwise_maximize(*args) == 0  # (the first call allocates the particle state)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    st = L.agp_pathwise_maximize(*args)
    host_ms = 1e3 * (time.perf_counter() - t0)
    e1.record()
    still_running = not e1.query()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1)
    print(f"host {host_ms:.3f} ms to enqueue, device {dev_ms:.3f} ms; still running at return: {still_running}")
    assert st == 0
    if not still_running:
        pytest.skip(f"the device finished first (device {dev_ms:.3f} ms, host {host_ms:.3f} ms): nothing to observe")
    assert host_ms < dev_ms


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _nan(torch, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _abi_outputs(torch, S, R, D):
    o = dict(X=_nan(torch, S, R, D), F=_nan(torch, S, R), xb=_nan(torch, S, D), fb=_nan(torch, S),
             ib=torch.full((S,), -7, dtype=torch.int64, device="cuda"))
    return o, {k: C.c_void_p(v.data_ptr()) for k, v in o.items()}


def _untouched(torch, o):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(o[k]).all()) for k in ("X", "F", "xb", "fb")) and bool((o["ib"] == -7).all())


def test_unsupported_is_refused_by_name(env):
    AGP, L, torch, capi = env["AGP"], env["L"], env["torch"], env["capi"]
    from agp_amd.pathwise import GRAD_REFUSAL_EXPONENTIAL

    for kind, D, word in (("exponential", 3, GRAD_REFUSAL_EXPONENTIAL), ("sqexponential", 65, "D > 64 is not supported")):
        model, Z = _model("svgp", 63, D, kind, 3.0 if D == 3 else M.ard(D))
        paths = AGP.sample_paths(model, 2, n_features=8, seed=1)
        x0 = torch.zeros(2, 4, D, dtype=torch.float64, device="cuda")
        o, p = _abi_outputs(torch, 2, 4, D)
        opts, keep = _opts(capi, 3, np.full(D, -1.0), np.full(D, 1.0), np.full(D, 0.1))
        st = L.agp_pathwise_maximize(paths._p, 0, C.c_void_p(x0.data_ptr()), D, 4, C.byref(opts), p["X"], D, p["F"], 4, p["xb"], D, p["fb"],
                                     p["ib"])
        msg = L.agp_last_error(model._ctx).decode()
        assert st == 5 and "agp_pathwise_maximize" in msg and word in msg, (st, msg)
        assert _untouched(torch, o)
        with pytest.raises(NotImplementedError, match=word):
            paths.maximize(np.zeros((4, D)), (-1.0, 1.0))


def test_argument_checks_through_the_abi(env):
    AGP, L, torch, capi = env["AGP"], env["L"], env["torch"], env["capi"]
    model, Z = _model("svgp", 64, 3, "sqexponential", 3.0)
    S, R, D = 2, 4, 3
    paths = AGP.sample_paths(model, S, n_features=8, seed=1)
    x0 = torch.zeros(S, R, D, dtype=torch.float64, device="cuda")
    o, p = _abi_outputs(torch, S, R, D)
    lo, hi, lr = np.full(D, -1.0), np.full(D, 1.0), np.full(D, 0.1)
    good = dict(latent=0, x0=C.c_void_p(x0.data_ptr()), ldx0=D, R=R, X=p["X"], ldxo=D, F=p["F"], ldf=R, xb=p["xb"], ldb=D, fb=p["fb"],
                ib=p["ib"], T=3, lo=lo, hi=hi, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, opts=True)
    nan1, inf1 = lo.copy(), hi.copy()
    nan1[1], inf1[2] = np.nan, np.inf
    cases = [("x0 must be given", dict(x0=None)), ("opts must be given", dict(opts=False)),
             ("at least one output must be given", dict(X=None, F=None, xb=None, fb=None, ib=None)),
             ("latent must lie in [0, n_latent)", dict(latent=1)), ("latent must lie in [0, n_latent)", dict(latent=-1)),
             ("n_starts >= 1", dict(R=0)), ("below 2^31", dict(R=2 ** 30, ldf=2 ** 30)),
             ("ldx0 >= D", dict(ldx0=2)), ("ldxo >= D", dict(ldxo=2)), ("ldf >= n_starts", dict(ldf=3)), ("ldb >= D", dict(ldb=2)),
             ("steps must lie in [0, 65536]", dict(T=-1)), ("steps must lie in [0, 65536]", dict(T=65537)),
             ("the bounds must be finite", dict(lo=nan1)), ("the bounds must be finite", dict(hi=inf1)),
             ("lo <= hi", dict(lo=hi + 1.0)),
             ("the step sizes must be finite and > 0", dict(lr=np.array([0.1, 0.0, 0.1]))),
             ("the step sizes must be finite and > 0", dict(lr=np.array([0.1, np.inf, 0.1]))),
             ("0 <= beta1, beta2 < 1", dict(beta1=1.0)), ("0 <= beta1, beta2 < 1", dict(beta2=-0.5)),
             ("eps must be finite and > 0", dict(eps=0.0)), ("eps must be finite and > 0", dict(eps=float("nan")))]
    for word, change in cases:
        a = {**good, **change}
        opts, keep = _opts(capi, a["T"], a["lo"], a["hi"], a["lr"], beta1=a["beta1"], beta2=a["beta2"], eps=a["eps"])
        st = L.agp_pathwise_maximize(paths._p, a["latent"], a["x0"], a["ldx0"], a["R"], C.byref(opts) if a["opts"] else None, a["X"],
                                     a["ldxo"], a["F"], a["ldf"], a["xb"], a["ldb"], a["fb"], a["ib"])
        msg = L.agp_last_error(model._ctx).decode()
        assert st == 1 and "agp_pathwise_maximize" in msg and word in msg, (word, st, msg)
        assert _untouched(torch, o), word
    opts, keep = _opts(capi, 3, lo, hi, lr)
    assert L.agp_pathwise_maximize(None, 0, good["x0"], D, R, C.byref(opts), p["X"], D, None, 0, None, 0, None, None) == 1  # p = NULL
    assert L.agp_pathwise_maximize(paths._p, 0, good["x0"], D, R, C.byref(opts), None, 0, p["F"], R, None, 0, None, None) == 0
    torch.cuda.synchronize()  # leading dimensions of outputs that are not given are not read
    assert not bool(torch.isnan(o["F"]).any()) and bool(torch.isnan(o["X"]).all())


def test_the_mirror_refuses_before_the_device_is_touched(env):
    """every refusal of the ABI raises from the mirror's host checks: the draw's device object is replaced by one that cannot be used"""
    AGP = env["AGP"]
    model, Z = _model("svgp", 64, 3, "sqexponential", 3.0)
    paths = AGP.sample_paths(model, 2, n_features=8, seed=1)
    real, paths._p = paths._p, object()  # any device call with it would raise a ctypes.ArgumentError
    try:
        x0 = np.zeros((4, 3))
        for exc, kw in ((ValueError, dict(latent=1)), (ValueError, dict(steps=-1)), (ValueError, dict(steps=65537)), (ValueError, dict(lr=0.0)),
                        (ValueError, dict(lr=[0.1, np.inf, 0.1])), (ValueError, dict(beta1=1.0)), (ValueError, dict(beta2=-0.5)),
                        (ValueError, dict(eps=0.0))):
            with pytest.raises(exc):
                paths.maximize(x0, (-1.0, 1.0), **kw)
        for X0, bounds in ((np.zeros((4, 2)), (-1.0, 1.0)), (np.zeros((0, 3)), (-1.0, 1.0)), (x0, (np.nan, 1.0)), (x0, (-1.0, np.inf)),
                           (x0, (1.0, -1.0))):
            with pytest.raises(ValueError):
                paths.maximize(X0, bounds)
    finally:
        paths._p = real
