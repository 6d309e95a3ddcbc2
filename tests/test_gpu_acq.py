"""The acquisition functions on the MI355X (include/agp_hip.h, "ACQUISITION FUNCTIONS"): agp_acq_moments against mpmath,
agp_svgp_acquisition and agp_svgp_acq_maximize against the NumPy restatement tests/_acq_ref.py fed with the DEVICE's own predictor
objects (model.predictor(): a trajectory amplifies the honest 1e-10 difference between the device's and the oracle's K^-1 beyond
PARITY, its own rounding it does not -- the conditioning is asserted first), bitwise repeatability, the box, the direction, the
layout contract, side effects, cache invalidation, the ABI's refusals and the two getters.

PARITY = 1e-8 is the project's parity bound; COND_CAP and GAP are those of the pathwise ascent.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _acq_ref as A
import _pathwise_max_ref as M
import _predgrad_cases as PC
from _pitched import Pitched
from test_acq_host import UCB_BETA, assert_close_rel, grid_moments, mp_point

pytestmark = pytest.mark.gpu

PARITY = A.PARITY
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, L=capi.lib(), torch=torch)


@functools.lru_cache(maxsize=None)
def _model_pc(pc_or_name):
    import agp_amd as AGP

    return A.make_model(AGP, pc_or_name)


def _model(name):
    """the trained device model of a case, shared by the tests that do not change it (cases on one model share it)"""
    first = next(n for n in A.CASES if A.CASES[n]["pc"] == A.CASES[name]["pc"])
    return _model_pc(first)


@functools.lru_cache(maxsize=None)
def _parts(name):
    return A.device_parts(_model(name), name)


def _py(AGP, q):
    return AGP.UCB(q["beta"]) if q["kind"] == "ucb" else (AGP.EI if q["kind"] == "ei" else AGP.PI)(q["best"], q["xi"])


def _svgp(model):
    return model._cur if hasattr(model, "_cur") else model


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _desc(capi, q):
    return capi.AcqDesc({"ucb": 0, "ei": 1, "pi": 2}[q["kind"]], int(q["s"] < 0), q["beta"], q["best"], q["xi"])


def _opts(capi, D, steps, lo, hi, lr, beta1=0.9, beta2=0.999, eps=1e-8, minimize=0, shared=0):
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (D,))) for v in (lo, hi, lr)]
    p = [k.ctypes.data_as(C.POINTER(C.c_double)) for k in keep]
    return capi.PwAscentOpts(steps, minimize, shared, beta1, beta2, eps, *p), keep


def _p(v):
    return C.c_void_p(v) if v else None


# ---- 1. the point function -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_moments_against_mpmath(env, kind, minimize):
    AGP = env["AGP"]
    s = -1.0 if minimize else 1.0
    mu, var = grid_moments()
    mu = s * mu
    acq = AGP.UCB(UCB_BETA) if kind == "ucb" else (AGP.EI if kind == "ei" else AGP.PI)(0.0, 0.0)
    al, dm, dv = AGP.acquisition_moments(acq, mu, var, minimize=minimize, grad=True)
    want = np.array([mp_point(kind, s, UCB_BETA, 0.0, 0.0, m, v) for m, v in zip(mu, var)]).T
    assert_close_rel(al, want[0], PARITY, f"{kind} alpha")
    assert_close_rel(dm, want[1], PARITY, f"{kind} d/dmu")
    assert_close_rel(dv * 2 * np.sqrt(var), want[2], PARITY, f"{kind} d/dsigma")
    assert _same(AGP.acquisition_moments(acq, mu, var, minimize=minimize), al)  # the derivatives are optional


def test_moments_zero_variance_and_nan(env):
    AGP = env["AGP"]
    mu = np.array([-1.0, 0.5, 0.5 + 1e-9, 2.0, np.nan, 0.3, np.nan])
    for v0 in (0.0, -1e-12):
        var = np.array([v0, v0, v0, v0, 1.0, np.nan, v0])
        for minimize in (False, True):
            for kind, acq in (("ucb", AGP.UCB(2.0)), ("ei", AGP.EI(0.5, 0.0)), ("pi", AGP.PI(0.5, 0.0))):
                got = AGP.acquisition_moments(acq, mu, var, minimize=minimize, grad=True)
                want = A.point(A.acq(kind, beta=2.0, best=0.5, minimize=minimize), mu, var)
                for g, w in zip(got, (want[0], want[1], want[3])):
                    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.all(np.isnan(g[4:]))
                    assert np.array_equal(g[:4], w[:4]), (kind, minimize, v0, g, w)  # the limits are exact


# ---- 2. acquisition(..., grad=True) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.CASES))
def test_acquisition_against_the_restatement(env, name):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    lat = A.CASES[name].get("latent", 0)
    Xt = A.data(name)["Xt"]
    X0, lo, hi, _ = A.inputs(name)
    for kind in A.KINDS:
        q = A.case_acq(kind, X0, parts, lo, hi)
        al, g = AGP.acquisition(model, _py(AGP, q), Xt, grad=True, latent=lat)
        wa, wg, _, _ = A.alpha_grad(q, Xt, parts)
        ea, eg = A.relerr(al, wa), A.relerr(g, wg)
        print(f"{name} {kind}: n_t = {len(Xt)}  alpha {ea:.2e}  grad {eg:.2e}")
        assert al.shape == (len(Xt),) and g.shape == Xt.shape and np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        assert ea <= PARITY and eg <= PARITY
        assert _same(AGP.acquisition(model, _py(AGP, q), Xt, latent=lat), al)  # values only: the same bits


def test_acquisition_crosses_the_chunk(env):
    name = "m130-d3-r4133"
    assert len(A.data(name)["Xt"]) == 4096 + 37  # (test_acquisition_against_the_restatement runs it)


@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "gp", "softmax-latent2"])
def test_ucb_reproduces_predict_f(env, name):
    AGP = env["AGP"]
    model, lat = _model(name), A.CASES[name].get("latent", 0)
    Xt = A.data(name)["Xt"]
    mu, var = AGP.predict_f(model, Xt, cov=True)
    if isinstance(mu, tuple):
        mu, var = mu[lat], var[lat]
    u0 = AGP.acquisition(model, AGP.UCB(0.0), Xt, latent=lat)
    u1 = AGP.acquisition(model, AGP.UCB(1.0), Xt, latent=lat)
    em, ev = A.relerr(u0, mu), A.relerr((u1 - u0) ** 2, var)
    print(f"{name}: UCB(0) against the mean {em:.2e}, (UCB(1) - UCB(0))^2 against the variance {ev:.2e}")
    assert em <= PARITY and ev <= PARITY
    assert _same(AGP.acquisition(model, AGP.UCB(0.0), Xt, latent=lat, minimize=True), -u0)


@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d1-m63-r63"])
def test_points_on_inducing_points(env, name):
    AGP = env["AGP"]
    assert A.spec(name)["kind"] in ("matern32", "matern52")
    model, parts = _model(name), _parts(name)
    Xt = np.vstack([parts[0], A.data(name)["Xt"][:1]])
    for kind in A.KINDS:
        q = A.acq(kind, beta=2.0, best=0.1, xi=A.XI)
        al, g = AGP.acquisition(model, _py(AGP, q), Xt, grad=True)
        wa, wg, _, _ = A.alpha_grad(q, Xt, parts)
        assert np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        assert A.relerr(al, wa) <= PARITY and A.relerr(g, wg) <= PARITY


# ---- 3. T = 0 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "m1-r1", "m130-d3-r4133"])
def test_zero_steps(env, name):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    q = A.case_acq("ei", X0, parts, lo, hi)
    xb, ab, ib, X, Al = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=0, lr=lr, full=True)
    clipped = np.minimum(np.maximum(X0, lo), hi)
    assert np.array_equal(X, clipped) and X0[0, 0] > hi[0]
    assert A.relerr(Al, A.alpha_grad(q, clipped, parts)[0]) <= PARITY
    wi, wx, wa = A.best(X, Al)
    assert int(ib) == wi and _same(xb, wx) and _same(ab, wa)


# ---- 4. trajectories -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,T", A.TRAJECTORIES)
def test_trajectories(env, name, kind, T):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    lat = A.CASES[name].get("latent", 0)
    X0, lo, hi, lr = A.inputs(name)
    q = A.case_acq(kind, X0, parts, lo, hi)
    wx, wa = A.ascent(q, X0, parts, lo, hi, lr, T)
    lx, la = A.ascent(q, X0, parts, lo, hi, lr, T, dtype=np.longdouble)
    box = float(np.max(hi - lo))
    cx, ca, gap = float(np.max(np.abs(wx - lx)) / box), A.relerr(wa, la), A.top_gap(wa)
    assert cx <= A.COND_CAP and ca <= A.COND_CAP, (cx, ca)  # on the device's own objects
    assert gap > A.GAP, gap
    xb, ab, ib, X, Al = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=T, lr=lr, latent=lat, full=True)
    ex, ea = float(np.max(np.abs(X - wx)) / box), A.relerr(Al, wa)
    wi, wbx, wba = A.best(wx, wa)
    print(f"{name} {kind} T={T}: conditioning x {cx:.1e} alpha {ca:.1e} gap {gap:.1e};  device x {ex:.2e} of the box, alpha {ea:.2e}")
    assert ex <= PARITY and ea <= PARITY
    assert int(ib) == wi
    assert float(np.max(np.abs(xb - wbx)) / box) <= PARITY and abs(float(ab) - wba) <= PARITY * np.max(np.abs(wa))
    x2, a2 = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=T, lr=lr, latent=lat)
    assert _same(x2, xb) and _same(a2, ab) and _same(xb, X[int(ib)]) and _same(ab, Al[int(ib)])


# ---- 5. bitwise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d64-m64-r64", "m130-d3-r4133"])
def test_bitwise(env, name):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    T = 1 if len(X0) > 4096 else 20
    acq = _py(AGP, A.case_acq("ei", X0, parts, lo, hi))
    r1 = AGP.maximize_acquisition(model, acq, X0, (lo, hi), steps=T, lr=lr, full=True)
    r2 = AGP.maximize_acquisition(model, acq, X0, (lo, hi), steps=T, lr=lr, full=True)
    assert all(_same(a, b) for a, b in zip(r1, r2))
    perm = np.random.default_rng(5).permutation(len(X0))
    r3 = AGP.maximize_acquisition(model, acq, X0[perm], (lo, hi), steps=T, lr=lr, full=True)
    if len(X0) <= 4096:  # (within one chunk a start has the same bits wherever it stands: the products in front pick one kernel)
        assert _same(r3[3], r1[3][perm]) and _same(r3[4], r1[4][perm])
    else:
        assert A.relerr(r3[3], r1[3][perm]) <= PARITY and A.relerr(r3[4], r1[4][perm]) <= PARITY
    again = AGP.acquisition(model, acq, r1[3])
    assert A.relerr(again, r1[4]) <= PARITY


# ---- 6. box and direction ------------------------------------------------------------------------------------------------------------------
def test_box(env):
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    lo, hi = lo.copy(), hi.copy()
    lo[1] = hi[1] = 0.25  # pinned
    acq = AGP.UCB(2.0)
    _, _, _, X, Al = AGP.maximize_acquisition(model, acq, X0, (lo, hi), steps=20, lr=lr, full=True)
    assert np.all(X >= lo) and np.all(X <= hi) and np.all(X[:, 1] == 0.25) and X0[0, 0] > hi[0] >= X[0, 0]
    wx, wa = A.ascent(A.acq("ucb", beta=2.0), X0, parts, lo, hi, lr, 20)
    assert float(np.max(np.abs(X - wx)) / np.max(hi - lo)) <= PARITY and A.relerr(Al, wa) <= PARITY


def test_minimize_is_the_maximisation_of_the_negated_model(env):
    """GP, BIT FOR BIT.  Why: the posterior of -y is the negated posterior -- the factor of K + sigma^2 I does not see y, and
    alpha = Sigma_y^-1 y is a chain of products and sums, each odd in y under round-to-nearest, so alpha' = -alpha to the bit -- and
    every operation between alpha and the outputs is odd or even in it with symmetric rounding: s (mu - best) = (-mu) - (-best),
    (s Phi) grad mu = Phi grad (-mu), the variance and its gradient do not see alpha at all, ADAM's v is even and its m odd in g."""
    AGP = env["AGP"]
    name = "gp"
    c, d = A.spec(name), A.data(name)
    pos = _model(name)
    neg = AGP.GP(d["X"], -d["y"], PC._akernel(AGP, c), noise=0.05, opt_noise=False, optimiser=False)
    X0, lo, hi, lr = A.inputs(name)
    mu = AGP.predict_f(pos, X0)
    for kind, mk in (("ucb", lambda b: AGP.UCB(2.0)), ("ei", lambda b: AGP.EI(b, A.XI)), ("pi", lambda b: AGP.PI(b, A.XI))):
        best = float(np.min(mu))
        r_min = AGP.maximize_acquisition(pos, mk(best), X0, (lo, hi), steps=20, lr=lr, minimize=True, full=True)
        r_neg = AGP.maximize_acquisition(neg, mk(-best), X0, (lo, hi), steps=20, lr=lr, full=True)
        assert all(_same(a, b) for a, b in zip(r_min, r_neg)), kind
        assert not _same(r_min[4], AGP.maximize_acquisition(pos, mk(best), X0, (lo, hi), steps=20, lr=lr, full=True)[4])


# ---- 7. 1-D sanity -------------------------------------------------------------------------------------------------------------------------
def test_one_d_beats_the_grid(env):
    AGP = env["AGP"]
    c = M.ONE_D
    X, y, X0, grid = M.one_d_data()
    k = c["sigma2"] * (AGP.Matern52Kernel() @ AGP.ScaleTransform(c["scale"]))
    model = AGP.GP(X, y, k, noise=c["noise"], opt_noise=False, optimiser=False)
    best = float(np.max(AGP.predict_f(model, X)))
    for acq in (AGP.UCB(2.0), AGP.EI(best, A.XI), AGP.PI(best, A.XI)):
        _, ab = AGP.maximize_acquisition(model, acq, X0, (c["lo"], c["hi"]), steps=c["T"], lr=c["lr"])
        on_grid = float(np.max(AGP.acquisition(model, acq, grid)))
        print(f"{acq}: device {float(ab):.6f}  grid {on_grid:.6f}")
        assert float(ab) >= on_grid


def test_best_none_takes_the_incumbent_from_the_data(env):
    AGP = env["AGP"]
    model, Xt = _model("gp"), A.data("gp")["Xt"]
    best = float(np.max(AGP.predict_f(model, model.X)))
    assert _same(AGP.acquisition(model, AGP.EI(xi=A.XI), Xt), AGP.acquisition(model, AGP.EI(best, A.XI), Xt))
    bmin = float(np.min(AGP.predict_f(model, model.X)))
    assert _same(AGP.acquisition(model, AGP.PI(), Xt, minimize=True), AGP.acquisition(model, AGP.PI(bmin), Xt, minimize=True))


# ---- 8. layout -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d64-m64-r64"])
def test_layout(env, name):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    R, D = X0.shape
    q = A.case_acq("ei", X0, parts, lo, hi)
    d = _desc(capi, q)
    h = model._ensure_handle(max(model._max_batch, 1))
    # agp_svgp_acquisition
    al, g = AGP.acquisition(model, _py(AGP, q), X0, grad=True)
    xin = Pitched("f64", data=X0, ld=D + 3, off=1, device="cuda")
    oa = Pitched("f64", rows=1, width=R, device="cuda")
    og = Pitched("f64", rows=R, width=D, ld=D + 5, off=1, device="cuda")
    assert L.agp_svgp_acquisition(h, 0, C.byref(d), _p(xin.ptr), D + 3, R, _p(oa.ptr), _p(og.ptr), D + 5) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xin, "xt"), (oa, "alpha_out"), (og, "grad_out")):
        b.check(w)
    assert not oa.unwritten().any() and not og.unwritten().any()
    assert _same(oa.window()[0], al) and _same(og.window(), g)
    # agp_svgp_acq_maximize
    ref = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=5, lr=lr, full=True)
    opts, keep = _opts(capi, D, 5, lo, hi, lr)
    ox = Pitched("f64", rows=R, width=D, ld=D + 2, off=1, device="cuda")
    oA = Pitched("f64", rows=1, width=R, off=1, device="cuda")
    bx = Pitched("f64", rows=1, width=D, off=1, device="cuda")
    ba = Pitched("f64", rows=1, width=1, device="cuda")
    bi = Pitched("i64", rows=1, width=1, device="cuda")
    assert L.agp_svgp_acq_maximize(h, 0, C.byref(d), _p(xin.ptr), D + 3, R, C.byref(opts), _p(ox.ptr), D + 2, _p(oA.ptr), _p(bx.ptr),
                                   _p(ba.ptr), _p(bi.ptr)) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xin, "x0"), (ox, "x_out"), (oA, "a_out"), (bx, "best_x"), (ba, "best_a"), (bi, "best_idx")):
        b.check(w)
        assert b is xin or not b.unwritten().any(), w
    assert _same(ox.window(), ref[3]) and _same(oA.window()[0], ref[4]) and _same(bx.window()[0], ref[0])
    assert _same(ba.window()[0, 0], ref[1]) and int(bi.window()[0, 0]) == int(ref[2])
    # NULL outputs: any subset
    ba2 = Pitched("f64", rows=1, width=1, device="cuda")
    assert L.agp_svgp_acq_maximize(h, 0, C.byref(d), _p(xin.ptr), D + 3, R, C.byref(opts), None, 0, None, None, _p(ba2.ptr), None) == 0
    L.agp_ctx_sync(model._ctx)
    ba2.check("best_a alone")
    assert _same(ba2.window()[0, 0], ref[1])
    ox2 = Pitched("f64", rows=R, width=D, ld=D + 2, device="cuda")
    assert L.agp_svgp_acq_maximize(h, 0, C.byref(d), _p(xin.ptr), D + 3, R, C.byref(opts), _p(ox2.ptr), D + 2, None, None, None, None) == 0
    L.agp_ctx_sync(model._ctx)
    ox2.check("x_out alone")
    assert _same(ox2.window(), ref[3])


# ---- 9. no side effects --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["svgp-logistic-m65-m32-ard", "svgp-softmax3-m65-sq-scale"])
def test_no_side_effects(env, pc):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    model, Xt = PC.make_model(AGP, pc), PC.data(pc)["Xt"]  # a model of its own: fresh caches
    lo, hi = np.full(3, -2.0), np.full(3, 2.0)

    def snapshot():
        terms = (C.c_double * 3)()
        model._chk(L.agp_svgp_elbo_terms(model._h, terms))
        snap = [np.asarray(tuple(terms))]
        for l in range(model.n_latent):
            snap += list(model.get_state(l))
            snap += [model.get_matrix(w, l) for w in (capi.VEC_THETA, capi.VEC_C, capi.VEC_MEAN_F)]
        return snap

    def preds(m):
        mu, var = AGP.predict_f(m, Xt, cov=True)
        return list(mu) + list(var) if isinstance(mu, tuple) else [mu, var]

    e0 = AGP.objective(model)
    before, p0 = snapshot(), preds(model)
    for lat in range(model.n_latent):
        AGP.acquisition(model, AGP.EI(0.1, A.XI), Xt, grad=True, latent=lat)
        AGP.acquisition(model, AGP.UCB(), Xt, latent=lat)
        AGP.maximize_acquisition(model, AGP.PI(0.1), Xt[:65], (lo, hi), steps=3, latent=lat)
    assert L.agp_svgp_check_status(model._h) == 0
    after, p1 = snapshot(), preds(model)
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.shape == b.shape and _same(a, b)
    assert all(_same(a, b) for a, b in zip(p0, p1))
    assert AGP.objective(model) == e0
    # ... and a call BEFORE the first prediction leaves the same predictions behind as none
    fresh = PC.make_model(AGP, pc)
    AGP.maximize_acquisition(fresh, AGP.EI(0.1), Xt[:65], (lo, hi), steps=2)
    assert all(_same(a, b) for a, b in zip(p0, preds(fresh)))


# ---- 10. the result follows the posterior ----------------------------------------------------------------------------------------------------
def test_new_posterior_new_result(env):
    AGP, L = env["AGP"], env["L"]
    name = "m65-logistic-m32-ard"
    pc = A.CASES[name]["pc"]
    model, d = PC.make_model(AGP, pc), PC.data(pc)
    X0, lo, hi, lr = A.inputs(name)

    def run():
        parts = A.device_parts(model, name)
        q = A.acq("ei", best=0.2, xi=A.XI)
        _, _, _, X, Al = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=20, lr=lr, full=True)
        wx, wa = A.ascent(q, X0, parts, lo, hi, lr, 20)
        assert float(np.max(np.abs(X - wx)) / np.max(hi - lo)) <= PARITY and A.relerr(Al, wa) <= PARITY
        return X, Al

    r0 = run()
    AGP.train_(model, d["X"], d["y"], 2, idx_stream=d["idx"][:2])
    r1 = run()
    assert not _same(r0[1], r1[1]) and A.relerr(r1[1], r0[1]) > 1e-6
    k = 1.1 * (AGP.Matern32Kernel() @ AGP.ARDTransform(np.array([1.4, 2.2, 0.9])))
    kd, keep = k.desc(3)
    model._chk(L.agp_svgp_set_kernel(model._h, 0, C.byref(kd)))
    model.kernels[0] = k
    r2 = run()
    assert not _same(r1[1], r2[1]) and A.relerr(r2[1], r1[1]) > 1e-6


# ---- 11. the ABI's refusals and argument checks ----------------------------------------------------------------------------------------------
def test_abi_refusals_and_argument_checks(env):
    AGP, L, capi, torch = env["AGP"], env["L"], env["capi"], env["torch"]
    rng = np.random.default_rng(0)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")

    def sparse(kernel, D, lik=None, T=np.float64):
        X = rng.standard_normal((40, D))
        y = np.where(X[:, 0] > 0, 1, -1)
        m = AGP.SVGP(kernel, lik or AGP.LogisticLikelihood(), AGP.AnalyticSVI(20), X[:6].copy(), optimiser=False, T=T)
        AGP.train_(m, X, y, 2)
        return m, X

    def both(model, X, desc, opts, latent=0, ldx=None, ldg=None, x_null=False, who=("agp_svgp_acquisition", "agp_svgp_acq_maximize")):
        """(status, message) of the two entry points; asserts that every output stayed NaN"""
        m = _svgp(model)
        h = m._ensure_handle(max(m._max_batch, 1))
        nt, D = X.shape
        Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
        outs = [nan(nt), nan(nt, D), nan(nt, D), nan(nt), nan(D), nan(1)]
        bi = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        xp = None if x_null else _p(Xd.data_ptr())
        res = []
        if "agp_svgp_acquisition" in who:
            st = L.agp_svgp_acquisition(h, latent, desc, xp, D if ldx is None else ldx, nt, _p(outs[0].data_ptr()), _p(outs[1].data_ptr()),
                                        D if ldg is None else ldg)
            res.append((st, L.agp_last_error(m._ctx).decode()))
        if "agp_svgp_acq_maximize" in who:
            st = L.agp_svgp_acq_maximize(h, latent, desc, xp, D if ldx is None else ldx, nt, opts, _p(outs[2].data_ptr()),
                                         D if ldg is None else ldg, _p(outs[3].data_ptr()), _p(outs[4].data_ptr()), _p(outs[5].data_ptr()),
                                         _p(bi.data_ptr()))
            res.append((st, L.agp_last_error(m._ctx).decode()))
        L.agp_ctx_sync(m._ctx)
        assert all(bool(torch.isnan(o).all()) for o in outs) and int(bi[0]) == -7
        return res

    def expect(res, status, text, who):
        for (st, msg), w in zip(res, who):
            assert st == status and w in msg and text in msg, (st, msg, w, text)

    names = ("agp_svgp_acquisition", "agp_svgp_acq_maximize")
    good = capi.AcqDesc(1, 0, 0.0, 0.1, 0.01)
    X2 = rng.standard_normal((40, 2))
    mc = AGP.MCGP(X2, np.where(X2[:, 0] > 0, 1, -1), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    mo = _model_mo(AGP)
    unsupported = [("AGP_F32", ) + sparse(AGP.SqExponentialKernel(), 3, T=np.float32),
                   ("ExponentialKernel", ) + sparse(AGP.ExponentialKernel(), 3),
                   ("at most 64", ) + sparse(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.2), 65),
                   ("AGP_FLAG_SAMPLED", mc, X2),
                   ("multi-output", mo, rng.standard_normal((40, 3)))]
    for text, model, X in unsupported:
        D = X.shape[1]
        opts, keep = _opts(capi, D, 3, -1.0, 1.0, 0.1)
        expect(both(model, X, C.byref(good), C.byref(opts)), UNSUPPORTED, text, names)
    model, X = sparse(AGP.Matern32Kernel(), 3)
    opts, keep = _opts(capi, 3, 3, -1.0, 1.0, 0.1)
    ok = C.byref(opts)
    expect(both(model, X, None, ok), INVALID, "desc must be given", names)
    for bad, text in ((capi.AcqDesc(3, 0, 0.0, 0.0, 0.0), "unknown kind"), (capi.AcqDesc(0, 0, -1.0, 0.0, 0.0), "beta >= 0"),
                      (capi.AcqDesc(1, 0, 0.0, 0.0, -0.5), "xi >= 0"), (capi.AcqDesc(1, 0, 0.0, float("inf"), 0.0), "finite"),
                      (capi.AcqDesc(0, 0, float("nan"), 0.0, 0.0), "finite")):
        expect(both(model, X, C.byref(bad), ok), INVALID, text, names)
    expect(both(model, X, C.byref(good), ok, latent=1), INVALID, "latent", names)
    expect(both(model, X, C.byref(good), ok, latent=-1), INVALID, "latent", names)
    expect(both(model, X, C.byref(good), ok, ldx=2), INVALID, "ld", names)
    expect(both(model, X, C.byref(good), ok, ldg=2), INVALID, "ld", names)
    expect(both(model, X, C.byref(good), ok, x_null=True), INVALID, "NULL", names[:1])
    mx = names[1:]
    expect(both(model, X, C.byref(good), ok, x_null=True, who=mx), INVALID, "x0 must be given", mx)
    expect(both(model, X, C.byref(good), None, who=mx), INVALID, "opts must be given", mx)
    for kw, text in ((dict(steps=-1), "steps"), (dict(steps=65537), "steps"), (dict(beta1=1.0), "beta1"), (dict(beta2=-0.1), "beta2"),
                     (dict(eps=0.0), "eps"), (dict(lo=1.0, hi=-1.0), "lo <= hi"), (dict(lo=float("-inf")), "finite"),
                     (dict(lr=0.0), "step sizes"), (dict(minimize=1), "opts->minimize"), (dict(shared=1), "x0_shared")):
        a = dict(steps=3, lo=-1.0, hi=1.0, lr=0.1)
        a.update(kw)
        o, keep = _opts(capi, 3, a.pop("steps"), a.pop("lo"), a.pop("hi"), a.pop("lr"), **a)
        expect(both(model, X, C.byref(good), C.byref(o), who=mx), INVALID, text, mx)
    o = capi.PwAscentOpts(3, 0, 0, 0.9, 0.999, 1e-8, None, None, None)
    expect(both(model, X, C.byref(good), C.byref(o), who=mx), INVALID, "lo_host", mx)
    h = model._ensure_handle(max(model._max_batch, 1))
    Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
    assert L.agp_svgp_acq_maximize(h, 0, C.byref(good), _p(Xd.data_ptr()), 3, 40, ok, None, 3, None, None, None, None) == INVALID
    assert "at least one output" in L.agp_last_error(model._ctx).decode()
    assert L.agp_svgp_acq_maximize(h, 0, C.byref(good), _p(Xd.data_ptr()), 3, 0, ok, None, 3, None, None, _p(Xd.data_ptr()), None) == INVALID
    assert "n_starts" in L.agp_last_error(model._ctx).decode()
    # n_t = 0 is a successful no-op, and the handle still works
    out = nan(40)
    assert L.agp_svgp_acquisition(h, 0, C.byref(good), _p(Xd.data_ptr()), 3, 0, _p(out.data_ptr()), None, 3) == 0
    L.agp_ctx_sync(model._ctx)
    assert bool(torch.isnan(out).all())
    assert L.agp_svgp_acquisition(h, 0, C.byref(good), _p(Xd.data_ptr()), 3, 40, _p(out.data_ptr()), None, 3) == 0
    L.agp_ctx_sync(model._ctx)
    assert not bool(torch.isnan(out).any())
    # agp_acq_moments
    mu, var, al = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.ones(4, dtype=torch.float64, device="cuda"), nan(4)
    ctx = model._ctx
    assert L.agp_acq_moments(ctx, None, 4, _p(mu.data_ptr()), _p(var.data_ptr()), _p(al.data_ptr()), None, None) == INVALID
    assert L.agp_acq_moments(ctx, C.byref(capi.AcqDesc(7, 0, 0.0, 0.0, 0.0)), 4, _p(mu.data_ptr()), _p(var.data_ptr()), _p(al.data_ptr()), None,
                             None) == INVALID
    assert "agp_acq_moments" in L.agp_last_error(ctx).decode() and "unknown kind" in L.agp_last_error(ctx).decode()
    assert L.agp_acq_moments(ctx, C.byref(good), 4, None, _p(var.data_ptr()), _p(al.data_ptr()), None, None) == INVALID
    assert L.agp_acq_moments(ctx, C.byref(good), -1, _p(mu.data_ptr()), _p(var.data_ptr()), _p(al.data_ptr()), None, None) == INVALID
    assert L.agp_acq_moments(ctx, C.byref(good), 0, None, None, None, None, None) == 0
    L.agp_ctx_sync(ctx)
    assert bool(torch.isnan(al).all())


def _model_mo(AGP):
    return PC.make_model(AGP, "mosvgp-2tasks-3latents-m63")


# ---- 12. the getters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "softmax-latent2", "vgp", "quadrature"])
def test_getters(env, name):
    """a = K^-1 mu and A = K^-1 - K^-1 Sigma K^-1 rebuilt on the host from get_state and AGP_MAT_KINV"""
    capi = env["capi"]
    model, lat = _model(name), A.CASES[name].get("latent", 0)
    a, Ap = model.predictor(lat)
    Kinv = model.get_matrix(capi.MAT_KINV, lat)
    st = model.get_state(lat)
    mu, Sig = st[0], st[1]
    wa, wA = Kinv @ mu, Kinv - Kinv @ Sig @ Kinv
    ea, eA = A.relerr(a, wa), A.relerr(Ap, wA)
    print(f"{name}: a {ea:.2e}  A {eA:.2e}")
    assert a.shape == (model.m,) and Ap.shape == (model.m, model.m)
    assert eA <= 1e-8 and ea <= 1e-8


def test_getters_exact_gp(env):
    """the exact GP: a = alpha (get_state's mu), A = Sigma_y^-1, the inverse of get_state's Sigma"""
    model = _model("gp")
    a, Ap = model.predictor()
    mu, Sig = model.get_state(0)[:2]
    assert _same(a, mu)
    assert A.relerr(Ap @ Sig, np.eye(model.m)) <= 1e-8
