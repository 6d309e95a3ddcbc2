"""Batch acquisition with pending points on the MI355X (include/agp_hip.h, "ACQUISITION FUNCTIONS", paragraph "Pending points"):
agp_svgp_acquisition_pending and agp_svgp_acq_maximize_batch against the NumPy restatement tests/_acq_batch_ref.py -- the DIRECT Schur
form, where the device computes the augmented predictor by bordering -- fed with the device's own predictor objects
(model.predictor()), the refit identity of the exact GP, the bit-level contract, side effects, the layout contract and the ABI's
refusals and argument checks.

PARITY = 1e-8 is the project's parity bound; COND_CAP and GAP are those of the pathwise ascent (tests/test_gpu_acq.py).  The
yardstick's own rounding on these inputs is 100 times below PARITY (tests/test_acq_batch_host.py).
"""
import ctypes as C

import numpy as np
import pytest

import _acq_batch_ref as B
import _acq_ref as A
import _predgrad_cases as PC
from _pitched import Pitched
from test_gpu_acq import _desc, _model, _model_mo, _opts, _p, _parts, _py, _same, _svgp, env  # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu

PARITY = A.PARITY
INVALID, UNSUPPORTED = 1, 5


def _lat(name):
    return A.CASES[name].get("latent", 0)


def _var(AGP, model, X, lat, **kw):
    """(mu, var) through UCB: UCB(0) = mu, (UCB(1) - UCB(0))^2 = var"""
    u0 = AGP.acquisition(model, AGP.UCB(0.0), X, latent=lat, **kw)
    u1 = AGP.acquisition(model, AGP.UCB(1.0), X, latent=lat, **kw)
    return u0, (u1 - u0) ** 2


# ---- 1. values and gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau2", B.NOISES)
@pytest.mark.parametrize("name", list(B.PENDING))
def test_pending_against_the_restatement(env, name, tau2):
    """The hard case is m1-r1 at noise 0: 63 pending points around one inducing point, one ON it and one a duplicate, cond(C) = 1.2e5,
    var_P <= 4e-3 at every test point.  An augmented A' summed into one matrix loses 1.7e-9 of the variance there and 4.5e-8 of EI; the
    device keeps the rank-one terms of the bordering apart (csrc/agp_acq_batch.h)."""
    AGP = env["AGP"]
    model, parts, lat = _model(name), _parts(name), _lat(name)
    P, X = B.pending(name), B.eval_points(name)
    X0, lo, hi, _ = A.inputs(name)
    assert len(X) == len(A.data(name)["Xt"]) + len(P)
    missed = []
    for kind in A.KINDS:
        q = A.case_acq(kind, X0, parts, lo, hi)
        al, g = AGP.acquisition(model, _py(AGP, q), X, grad=True, latent=lat, pending=P, pending_noise=tau2)
        wa, wg, _, _ = B.alpha_grad(q, X, parts, P, tau2)
        ea, eg = A.relerr(al, wa), A.relerr(g, wg)
        print(f"{name} {kind} tau2={tau2}: m' = {len(parts[0])} + {len(P)}, n_t = {len(X)}  alpha {ea:.2e}  grad {eg:.2e}")
        assert al.shape == (len(X),) and g.shape == X.shape and np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        if not (ea <= PARITY and eg <= PARITY):
            missed.append((kind, ea, eg))
        assert _same(AGP.acquisition(model, _py(AGP, q), X, latent=lat, pending=P, pending_noise=tau2), al)  # values only
    assert not missed, missed  # (every kind is measured and printed before the first miss stops the test)


def test_pending_crosses_the_chunk_and_the_tiles(env):
    assert len(B.eval_points("m130-d3-r4133")) > 4096  # (test_pending_against_the_restatement runs it)
    mps = {A.spec(n)["m"] + k for n, k in B.PENDING.items() if A.spec(n)["m"]}
    assert {64, 65} <= mps and B.PENDING["m1-r1"] == 63


# ---- 2. the refit identity ----------------------------------------------------------------------------------------------------------------------
def test_refit_identity_on_the_device(env):
    """GP with noise sigma^2 and pending_noise = sigma^2: the GP rebuilt on (X u P, y u mu(P)), nothing optimised"""
    AGP = env["AGP"]
    name, noise = "gp", 0.05
    model, c, d = _model(name), A.spec(name), A.data(name)
    P, Xt = B.pending(name), B.eval_points(name)
    muP = AGP.predict_f(model, P)
    second = AGP.GP(np.vstack([d["X"], P]), np.concatenate([d["y"], muP]), PC._akernel(AGP, c), noise=noise, opt_noise=False, optimiser=False)
    mu2, var2 = AGP.predict_f(second, Xt, cov=True)
    u0, var = _var(AGP, model, Xt, 0, pending=P, pending_noise=noise)
    em, ev = A.relerr(u0, mu2), A.relerr(var, var2)
    print(f"refit: UCB(0) against the second model's mean {em:.2e}, (UCB(1) - UCB(0))^2 against its variance {ev:.2e}")
    assert em <= PARITY and ev <= PARITY


# ---- 3. sanity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gp", "m65-logistic-m32-ard", "m1-r1", "d64-m64-r64"])
def test_the_variance_shrinks(env, name):
    """var_P <= var at every test point and, with noise 0, var_P(p_i) <= 2 jitter + PARITY at every pending point"""
    AGP = env["AGP"]
    model, lat = _model(name), _lat(name)
    P, X = B.pending(name), B.eval_points(name)
    mu, var = _var(AGP, model, X, lat)
    for tau2 in B.NOISES:
        mu_p, var_p = _var(AGP, model, X, lat, pending=P, pending_noise=tau2)
        print(f"{name} tau2={tau2}: max (var_P - var) {float(np.max(var_p - var)):.2e}, at the pending points max var_P "
              f"{float(np.max(var_p[-len(P):])):.3e}")
        assert _same(mu_p, mu)  # the mean stays: a' = [a; 0]
        assert np.all(var_p <= var)
        if tau2 == 0.0:
            assert np.all(var_p[-len(P):] <= 2 * A.JITTER + PARITY)


# ---- 4. the batch ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.BATCHES, ids=B.batch_id)
def test_batch_against_the_restatement(env, case):
    AGP = env["AGP"]
    name, kind, tau2, npend, nq, T = case
    model, parts, lat = _model(name), _parts(name), _lat(name)
    X0, lo, hi, lr = A.inputs(name)
    q = A.case_acq(kind, X0, parts, lo, hi)
    P = B.pending(name, npend) if npend else None
    Pr = P if npend else np.zeros((0, X0.shape[1]))
    r64 = B.batch(q, nq, X0, parts, Pr, tau2, lo, hi, lr, T)
    rld = B.batch(q, nq, X0, parts, Pr, tau2, lo, hi, lr, T, dtype=np.longdouble)
    cx, ca, gap, same = B.conditioning(r64, rld, lo, hi)
    assert cx <= A.COND_CAP and ca <= A.COND_CAP, (cx, ca)  # on the device's own objects
    assert gap > A.GAP and same, (gap, same)
    Xb, ab, ib = AGP.maximize_acquisition_batch(model, _py(AGP, q), nq, X0, (lo, hi), pending=P, pending_noise=tau2, steps=T, lr=lr,
                                                latent=lat, full=True)
    assert Xb.shape == (nq, X0.shape[1]) and ab.shape == (nq,) and ib.shape == (nq,) and ib.dtype == np.int64
    box = float(np.max(hi - lo))
    wx, wa, wi = np.array([r["x"] for r in r64]), np.array([r["a"] for r in r64]), [r["idx"] for r in r64]
    scale = max(float(np.max(np.abs(r["A"]))) for r in r64)
    ex, ea = float(np.max(np.abs(Xb - wx))) / box, float(np.max(np.abs(ab - wa))) / scale
    print(f"{B.batch_id(case)}: conditioning x {cx:.1e} alpha {ca:.1e} gap {gap:.1e};  device idx {[int(i) for i in ib]} (want {wi}), x {ex:.2e} of "
          f"the box, alpha {ea:.2e}")
    assert [int(i) for i in ib] == wi
    assert ex <= PARITY and ea <= PARITY
    assert np.all(Xb >= lo) and np.all(Xb <= hi)


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d64-m64-r64"])
def test_bit_level_contract(env, name):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    D = X0.shape[1]
    X, P = B.eval_points(name), B.pending(name, 3)
    acq = _py(AGP, A.case_acq("ei", X0, parts, lo, hi))
    none = np.zeros((0, D))
    # n_pending = 0: the bits of agp_svgp_acquisition
    al, g = AGP.acquisition(model, acq, X, grad=True)
    al0, g0 = AGP.acquisition(model, acq, X, grad=True, pending=none, pending_noise=0.3)
    assert _same(al0, al) and _same(g0, g)
    # n_pending = 0, q = 1: the bits of agp_svgp_acq_maximize
    kw = dict(steps=20, lr=lr)
    xb, ab, ib = AGP.maximize_acquisition(model, acq, X0, (lo, hi), full=True, **kw)[:3]
    X1, a1, i1 = AGP.maximize_acquisition_batch(model, acq, 1, X0, (lo, hi), full=True, pending_noise=0.3, **kw)
    assert _same(X1[0], xb) and _same(a1[0], ab) and int(i1[0]) == int(ib)
    # a batch of q = q chained calls with q = 1, each given the earlier winners as extra pending points; and a repeat
    for pend, tau2 in ((None, 0.0), (P, 0.01)):
        full = AGP.maximize_acquisition_batch(model, acq, 4, X0, (lo, hi), pending=pend, pending_noise=tau2, full=True, **kw)
        again = AGP.maximize_acquisition_batch(model, acq, 4, X0, (lo, hi), pending=pend, pending_noise=tau2, full=True, **kw)
        assert all(_same(a, b) for a, b in zip(full, again))
        cur = none if pend is None else pend
        for b in range(4):
            one = AGP.maximize_acquisition_batch(model, acq, 1, X0, (lo, hi), pending=cur, pending_noise=tau2, full=True, **kw)
            assert _same(one[0][0], full[0][b]) and _same(one[1][0], full[1][b]) and int(one[2][0]) == int(full[2][b]), (b, tau2)
            cur = np.vstack([cur, one[0]])
        assert len({tuple(x) for x in full[0]}) > 1  # (the rounds do not all return one point)
        # a permutation of the starts within one chunk: the same batch points
        perm = np.random.default_rng(5).permutation(len(X0))
        pb = AGP.maximize_acquisition_batch(model, acq, 4, X0[perm], (lo, hi), pending=pend, pending_noise=tau2, full=True, **kw)
        assert _same(pb[0], full[0]) and _same(pb[1], full[1]) and [int(perm[i]) for i in pb[2]] == [int(i) for i in full[2]]
    # the values with pending points repeat, too, and do not depend on what ran in between
    v1 = AGP.acquisition(model, acq, X, grad=True, pending=P, pending_noise=0.01)
    AGP.maximize_acquisition_batch(model, acq, 2, X0, (lo, hi), steps=2, lr=lr)
    v2 = AGP.acquisition(model, acq, X, grad=True, pending=P, pending_noise=0.01)
    assert _same(v1[0], v2[0]) and _same(v1[1], v2[1])


# ---- 6. no side effects ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["svgp-logistic-m65-m32-ard", "svgp-softmax3-m65-sq-scale"])
def test_no_side_effects(env, pc):
    AGP, L = env["AGP"], env["L"]
    model, Xt = PC.make_model(AGP, pc), PC.data(pc)["Xt"]  # a model of its own: fresh caches
    lo, hi = np.full(3, -2.0), np.full(3, 2.0)
    P = Xt[200:205]

    def snapshot():
        snap = []
        mu, var = AGP.predict_f(model, Xt, cov=True)
        snap += list(mu) + list(var) if isinstance(mu, tuple) else [mu, var]
        gm, gv = AGP.predict_f_grad(model, Xt, cov=True)
        snap += list(gm) + list(gv) if isinstance(gm, (tuple, list)) else [gm, gv]
        for lat in range(model.n_latent):
            snap += list(AGP.acquisition(model, AGP.EI(0.1, A.XI), Xt, grad=True, latent=lat))
            snap += list(AGP.maximize_acquisition(model, AGP.UCB(), Xt[:65], (lo, hi), steps=3, latent=lat, full=True))
            snap += [np.asarray(t) for t in model.get_state(lat)]
            snap += list(model.predictor(lat))
        return snap

    before = snapshot()
    for lat in range(model.n_latent):
        AGP.acquisition(model, AGP.EI(0.1, A.XI), Xt, grad=True, latent=lat, pending=P, pending_noise=0.01)
        AGP.maximize_acquisition_batch(model, AGP.PI(0.1), 3, Xt[:65], (lo, hi), steps=3, latent=lat, pending=P)
    assert L.agp_svgp_check_status(model._h) == 0
    after = snapshot()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert np.shape(a) == np.shape(b) and _same(a, b)
    # ... and the new calls BEFORE the first prediction leave the same predictions behind as none
    fresh = PC.make_model(AGP, pc)
    AGP.maximize_acquisition_batch(fresh, AGP.EI(0.1), 2, Xt[:65], (lo, hi), steps=2, pending=P)
    AGP.acquisition(fresh, AGP.UCB(), Xt, pending=P)
    mu, var = AGP.predict_f(fresh, Xt, cov=True)
    now = list(mu) + list(var) if isinstance(mu, tuple) else [mu, var]
    assert all(_same(a, b) for a, b in zip(before, now))


# ---- 7. layout ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d64-m64-r64"])
def test_layout(env, name):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    R, D = X0.shape
    P, tau2, nq = B.pending(name, 3), 0.01, 3
    q = A.case_acq("ei", X0, parts, lo, hi)
    d = _desc(capi, q)
    h = model._ensure_handle(max(model._max_batch, 1))
    # agp_svgp_acquisition_pending
    al, g = AGP.acquisition(model, _py(AGP, q), X0, grad=True, pending=P, pending_noise=tau2)
    xp = Pitched("f64", data=P, ld=D + 1, off=1, device="cuda")
    xin = Pitched("f64", data=X0, ld=D + 3, off=1, device="cuda")
    oa = Pitched("f64", rows=1, width=R, device="cuda")
    og = Pitched("f64", rows=R, width=D, ld=D + 5, off=1, device="cuda")
    assert L.agp_svgp_acquisition_pending(h, 0, C.byref(d), _p(xp.ptr), D + 1, len(P), tau2, _p(xin.ptr), D + 3, R, _p(oa.ptr), _p(og.ptr),
                                          D + 5) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xp, "xp"), (xin, "xt"), (oa, "alpha_out"), (og, "grad_out")):
        b.check(w)
    assert not oa.unwritten().any() and not og.unwritten().any()
    assert _same(oa.window()[0], al) and _same(og.window(), g)
    # agp_svgp_acq_maximize_batch
    ref = AGP.maximize_acquisition_batch(model, _py(AGP, q), nq, X0, (lo, hi), pending=P, pending_noise=tau2, steps=5, lr=lr, full=True)
    opts, keep = _opts(capi, D, 5, lo, hi, lr)
    ox = Pitched("f64", rows=nq, width=D, ld=D + 2, off=1, device="cuda")
    oA = Pitched("f64", rows=1, width=nq, off=1, device="cuda")
    oi = Pitched("i64", rows=1, width=nq, off=1, device="cuda")
    assert L.agp_svgp_acq_maximize_batch(h, 0, C.byref(d), _p(xp.ptr), D + 1, len(P), tau2, nq, _p(xin.ptr), D + 3, R, C.byref(opts),
                                         _p(ox.ptr), D + 2, _p(oA.ptr), _p(oi.ptr)) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xp, "xp"), (xin, "x0"), (ox, "xb_out"), (oA, "ab_out"), (oi, "idxb_out")):
        b.check(w)
        assert b in (xp, xin) or not b.unwritten().any(), w
    assert _same(ox.window(), ref[0]) and _same(oA.window()[0], ref[1]) and np.array_equal(oi.window()[0], ref[2])
    # the nullable outputs left out
    ox2 = Pitched("f64", rows=nq, width=D, ld=D + 2, device="cuda")
    assert L.agp_svgp_acq_maximize_batch(h, 0, C.byref(d), _p(xp.ptr), D + 1, len(P), tau2, nq, _p(xin.ptr), D + 3, R, C.byref(opts),
                                         _p(ox2.ptr), D + 2, None, None) == 0
    L.agp_ctx_sync(model._ctx)
    ox2.check("xb_out alone")
    assert _same(ox2.window(), ref[0])
    assert L.agp_svgp_check_status(h) == 0


# ---- 8. the ABI's refusals and argument checks ------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_argument_checks(env):
    AGP, L, capi, torch = env["AGP"], env["L"], env["capi"], env["torch"]
    rng = np.random.default_rng(0)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    names = ("agp_svgp_acquisition_pending", "agp_svgp_acq_maximize_batch")

    def sparse(kernel, D, T=np.float64):
        X = rng.standard_normal((40, D))
        y = np.where(X[:, 0] > 0, 1, -1)
        m = AGP.SVGP(kernel, AGP.LogisticLikelihood(), AGP.AnalyticSVI(20), X[:6].copy(), optimiser=False, T=T)
        AGP.train_(m, X, y, 2)
        return m, X

    def both(model, X, desc, opts, latent=0, n=2, noise=0.0, q=2, ldp=None, ldx=None, ldg=None, ldxb=None, xp_null=False, x_null=False,
             xb_null=False, who=names):
        """(status, message) of the two entry points; asserts that every output kept its sentinel"""
        m = _svgp(model)
        h = m._ensure_handle(max(m._max_batch, 1))
        nt, D = X.shape
        Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
        Pd = torch.as_tensor(X[:max(n, 1)], dtype=torch.float64, device="cuda").contiguous()
        outs = [nan(nt), nan(nt, D), nan(64, D), nan(64)]
        bi = torch.full((64,), -7, dtype=torch.int64, device="cuda")
        xp = None if xp_null else _p(Pd.data_ptr())
        x = None if x_null else _p(Xd.data_ptr())
        ld = lambda v: D if v is None else v
        res = []
        if names[0] in who:
            st = L.agp_svgp_acquisition_pending(h, latent, desc, xp, ld(ldp), n, noise, x, ld(ldx), nt, _p(outs[0].data_ptr()),
                                                _p(outs[1].data_ptr()), ld(ldg))
            res.append((st, L.agp_last_error(m._ctx).decode()))
        if names[1] in who:
            st = L.agp_svgp_acq_maximize_batch(h, latent, desc, xp, ld(ldp), n, noise, q, x, ld(ldx), nt, opts,
                                               None if xb_null else _p(outs[2].data_ptr()), ld(ldxb), _p(outs[3].data_ptr()),
                                               _p(bi.data_ptr()))
            res.append((st, L.agp_last_error(m._ctx).decode()))
        L.agp_ctx_sync(m._ctx)
        assert all(bool(torch.isnan(o).all()) for o in outs) and bool((bi == -7).all())
        return res

    def expect(res, status, text, who=names):
        assert len(res) == len(who)
        for (st, msg), w in zip(res, who):
            assert st == status and w + ":" in msg and text in msg, (st, msg, w, text)

    good = capi.AcqDesc(1, 0, 0.0, 0.1, 0.01)
    X2 = rng.standard_normal((40, 2))
    mc = AGP.MCGP(X2, np.where(X2[:, 0] > 0, 1, -1), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    unsupported = [("AGP_F32 handles are not supported (the acquisition functions are Float64)", ) + sparse(AGP.SqExponentialKernel(), 3, T=np.float32),
                   ("ExponentialKernel is not differentiable at zero distance", ) + sparse(AGP.ExponentialKernel(), 3),
                   ("the input dimension D must be at most 64", ) + sparse(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.2), 65),
                   ("Gibbs-sampled models (AGP_FLAG_SAMPLED) are not supported", mc, X2),
                   ("multi-output handles (MOSVGP, MOVGP) are not supported", _model_mo(AGP), rng.standard_normal((40, 3)))]
    for text, model, X in unsupported:  # the words of agp_svgp_acquisition / agp_svgp_acq_maximize
        opts, keep = _opts(capi, X.shape[1], 3, -1.0, 1.0, 0.1)
        expect(both(model, X, C.byref(good), C.byref(opts)), UNSUPPORTED, text)
    model, X = sparse(AGP.Matern32Kernel(), 3)
    opts, keep = _opts(capi, 3, 3, -1.0, 1.0, 0.1)
    ok, gd = C.byref(opts), C.byref(good)
    # what the two new calls add
    expect(both(model, X, gd, ok, n=-1), INVALID, "n_pending")
    expect(both(model, X, gd, ok, n=64), INVALID, "n_pending")  # 64 + 1 and 64 + 2
    expect(both(model, X, gd, ok, n=40, q=25, who=names[1:]), INVALID, "n_pending", names[1:])
    expect(both(model, X, gd, ok, q=0, who=names[1:]), INVALID, "q >= 1", names[1:])
    expect(both(model, X, gd, ok, q=65, n=0, who=names[1:]), INVALID, "q >= 1", names[1:])
    for bad in (-0.5, float("nan"), float("inf")):
        expect(both(model, X, gd, ok, noise=bad), INVALID, "noise")
    expect(both(model, X, gd, ok, xp_null=True), INVALID, "xp must be given")
    expect(both(model, X, gd, ok, ldp=2), INVALID, "ldp >= D")
    expect(both(model, X, gd, ok, ldxb=2, who=names[1:]), INVALID, "ldxb >= D", names[1:])
    expect(both(model, X, gd, ok, xb_null=True, who=names[1:]), INVALID, "xb_out must be given", names[1:])
    # what the existing two already check
    expect(both(model, X, None, ok), INVALID, "desc must be given")
    for bad, text in ((capi.AcqDesc(3, 0, 0.0, 0.0, 0.0), "unknown kind"), (capi.AcqDesc(0, 0, -1.0, 0.0, 0.0), "beta >= 0"),
                      (capi.AcqDesc(1, 0, 0.0, 0.0, -0.5), "xi >= 0"), (capi.AcqDesc(1, 0, 0.0, float("inf"), 0.0), "finite"),
                      (capi.AcqDesc(0, 0, float("nan"), 0.0, 0.0), "finite")):
        expect(both(model, X, C.byref(bad), ok), INVALID, text)
    expect(both(model, X, gd, ok, latent=1), INVALID, "latent")
    expect(both(model, X, gd, ok, latent=-1), INVALID, "latent")
    expect(both(model, X, gd, ok, ldx=2), INVALID, "ld")
    expect(both(model, X, gd, ok, ldg=2, who=names[:1]), INVALID, "ldg", names[:1])
    expect(both(model, X, gd, ok, x_null=True, who=names[:1]), INVALID, "NULL", names[:1])
    mx = names[1:]
    expect(both(model, X, gd, ok, x_null=True, who=mx), INVALID, "x0 must be given", mx)
    expect(both(model, X, gd, None, who=mx), INVALID, "opts must be given", mx)
    for kw, text in ((dict(steps=-1), "steps"), (dict(steps=65537), "steps"), (dict(beta1=1.0), "beta1"), (dict(beta2=-0.1), "beta2"),
                     (dict(eps=0.0), "eps"), (dict(lo=1.0, hi=-1.0), "lo <= hi"), (dict(lo=float("-inf")), "finite"),
                     (dict(lr=0.0), "step sizes"), (dict(minimize=1), "opts->minimize"), (dict(shared=1), "x0_shared")):
        a = dict(steps=3, lo=-1.0, hi=1.0, lr=0.1)
        a.update(kw)
        o, keep = _opts(capi, 3, a.pop("steps"), a.pop("lo"), a.pop("hi"), a.pop("lr"), **a)
        expect(both(model, X, gd, C.byref(o), who=mx), INVALID, text, mx)
    o = capi.PwAscentOpts(3, 0, 0, 0.9, 0.999, 1e-8, None, None, None)
    expect(both(model, X, gd, C.byref(o), who=mx), INVALID, "lo_host", mx)
    h = model._ensure_handle(max(model._max_batch, 1))
    Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
    out = nan(40, 3)
    assert L.agp_svgp_acq_maximize_batch(h, 0, gd, None, 3, 0, 0.0, 1, _p(Xd.data_ptr()), 3, 0, ok, _p(out.data_ptr()), 3, None, None) == INVALID
    assert "n_starts" in L.agp_last_error(model._ctx).decode()
    # n_t = 0 is a successful no-op; xp NULL with n_pending = 0 is fine; and the handle still works, with nothing latched
    al = nan(40)
    assert L.agp_svgp_acquisition_pending(h, 0, gd, _p(Xd.data_ptr()), 3, 2, 0.0, _p(Xd.data_ptr()), 3, 0, _p(al.data_ptr()), None, 3) == 0
    L.agp_ctx_sync(model._ctx)
    assert bool(torch.isnan(al).all()) and bool(torch.isnan(out).all())
    assert L.agp_svgp_acquisition_pending(h, 0, gd, None, 3, 0, 0.0, _p(Xd.data_ptr()), 3, 40, _p(al.data_ptr()), None, 3) == 0
    assert L.agp_svgp_acq_maximize_batch(h, 0, gd, None, 3, 0, 0.0, 2, _p(Xd.data_ptr()), 3, 40, ok, _p(out.data_ptr()), 3, None, None) == 0
    L.agp_ctx_sync(model._ctx)
    assert not bool(torch.isnan(al).any()) and not bool(torch.isnan(out[:2]).any()) and bool(torch.isnan(out[2:]).all())
    assert L.agp_svgp_check_status(h) == 0
