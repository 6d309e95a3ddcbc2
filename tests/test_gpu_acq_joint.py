"""Joint Monte-Carlo batch acquisition on the MI355X (include/agp_hip.h, "ACQUISITION FUNCTIONS", paragraph "Joint batches"):
agp_svgp_acquisition_joint and agp_svgp_acq_maximize_joint against the NumPy restatement tests/_acq_joint_ref.py, fed with the DEVICE's
own predictor objects (model.predictor()) and the same base samples.  Every comparison runs on inputs whose kink margin -- in the
restatement, on those very objects -- exceeds J.KINK; tests/test_acq_joint_host.py asserts the same, and the restatement's own
rounding, on the oracle's objects.  No case is left out.

PARITY = 1e-8 is the project's parity bound; COND_CAP and GAP are those of the pathwise ascent.
"""
import ctypes as C

import numpy as np
import pytest

import _acq_joint_ref as J
import _acq_ref as A
from _pitched import Pitched
from test_acq_joint_host import DEGENERATE_GRAD
from test_gpu_acq import _desc, _model, _model_mo, _opts, _p, _parts, _same, _svgp

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


def _py(AGP, q):
    return AGP.UCB(q["beta"]) if q["kind"] == "ucb" else AGP.EI(q["best"], q["xi"])


def _kw(q, P, eps):
    return dict(base_samples=eps, pending=P if len(P) else None, minimize=q["s"] < 0)


# ---- 1. values and gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", J.VALUES, ids=J.value_id)
def test_values_and_gradients_against_the_restatement(env, case):
    AGP = env["AGP"]
    name, q, n, S, nsets, seed = case
    model, parts = _model(name), _parts(name)
    X, P = J.sets(name, q, n, nsets, seed)
    eps = J.table(S, q + n, seed)
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, X, P, parts)
        wa, wg, margin = J.alpha_grad(acq, X, parts, eps, P)
        assert float(np.min(margin)) > J.KINK, (kind, minimize, float(np.min(margin)))  # every set: none is left out
        al, g = AGP.acquisition_joint(model, _py(AGP, acq), X, grad=True, **_kw(acq, P, eps))
        ea, eg = A.relerr(al, wa), A.relerr(g, wg)
        print(f"{J.value_id(case)} {kind} minimize={minimize}: margin {float(np.min(margin)):.1e}  alpha {ea:.2e}  grad {eg:.2e}")
        assert al.shape == (nsets,) and g.shape == X.shape and np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        assert ea <= PARITY and eg <= PARITY
        assert _same(AGP.acquisition_joint(model, _py(AGP, acq), X, **_kw(acq, P, eps)), al)  # values only: the same bits
    a1, g1 = AGP.acquisition_joint(model, _py(AGP, acq), X[0], grad=True, **_kw(acq, P, eps))  # one tuple (q, D): a scalar
    assert a1.shape == () and g1.shape == X[0].shape and _same(a1, al[0]) and _same(g1, g[0])


def test_the_mirror_draws_the_restated_table(env):
    """without base_samples the mirror fills the table with agp_mc_normals(seed, t=0, stream=3): the same bits as the restated one"""
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model, parts = _model(name), _parts(name)
    X, P = J.sets(name, 3, 1, 5, 0)
    assert _same(AGP.mc_normals(5, 0, J.STREAM, 64, 4), J.base_samples(64, 4, 5))
    acq = J.case_acq("ei", False, X, P, parts)
    got = AGP.acquisition_joint(model, _py(AGP, acq), X, samples=64, seed=5, pending=P)
    assert _same(got, AGP.acquisition_joint(model, _py(AGP, acq), X, base_samples=J.base_samples(64, 4, 5), pending=P))
    assert not _same(got, AGP.acquisition_joint(model, _py(AGP, acq), X, samples=64, seed=6, pending=P))


# ---- 2. C against agp_svgp_predict_f_cov ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "gp", "d64-m64-r64"])
def test_covariance_against_predict_f_cov(env, name):
    """mu and C are recovered from the device through the criteria themselves, with one sample.  One member, eps = 1: q-UCB(0) = mu and
    q-UCB(1) - q-UCB(0) = sqrt(pi/2) sigma.  Two members, eps = (1, 0): f = (mu_0 + L_00, mu_1 + L_10), and q-EI with a far incumbent
    gives max(f) + 20 when maximising and 20 - min(f) when minimising, so their sum is f_0 + f_1 whichever member wins and
    C_10 = L_10 L_00 follows.  Compared within PARITY, not bit for bit: the joint kernel sums over m with the lanes of a wave strided
    and a butterfly, acquisition(UCB) in ascending tiles, and agp_svgp_predict_f_cov by a GEMM."""
    AGP = env["AGP"]
    model = _model(name)
    X, _ = J.sets(name, 2, 0, 24, 2)
    pts = X.reshape(-1, X.shape[2])
    mu, cov = AGP.predict_f(model, pts, cov=True, diag=False)
    one = np.ones((1, 1))
    m0 = AGP.acquisition_joint(model, AGP.UCB(0.0), pts[:, None, :], base_samples=one)
    m1 = AGP.acquisition_joint(model, AGP.UCB(1.0), pts[:, None, :], base_samples=one)
    sg = (m1 - m0) / np.sqrt(np.pi / 2)
    u0, u1 = AGP.acquisition(model, AGP.UCB(0.0), pts), AGP.acquisition(model, AGP.UCB(1.0), pts)
    e_mu, e_var = A.relerr(m0, mu), A.relerr(sg * sg, np.diag(cov))
    e_ucb = max(A.relerr(m0, u0), A.relerr(sg, u1 - u0))
    e = np.array([[1.0, 0.0]])
    hi = AGP.acquisition_joint(model, AGP.EI(-20.0), X, base_samples=e)
    lo = AGP.acquisition_joint(model, AGP.EI(20.0), X, base_samples=e, minimize=True)
    fsum = (hi - 20.0) + (20.0 - lo)
    m0, sg = m0.reshape(-1, 2), sg.reshape(-1, 2)
    c10 = (fsum - m0[:, 0] - m0[:, 1] - sg[:, 0]) * sg[:, 0]
    want = np.array([cov[2 * r + 1, 2 * r] for r in range(len(X))])
    e_off = float(np.max(np.abs(c10 - want)) / np.max(np.abs(cov)))
    print(f"{name}: mu {e_mu:.2e}  diag C {e_var:.2e}  against acquisition(UCB) {e_ucb:.2e}  off-diagonal {e_off:.2e}")
    assert e_mu <= PARITY and e_var <= PARITY and e_ucb <= PARITY and e_off <= PARITY
    assert np.max(np.abs(want)) > 1e-3 * np.max(np.abs(cov))  # (the off-diagonal entries are not noise)


# ---- 3. q = 1, n = 0 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ei", "ucb"])
def test_one_member(env, kind):
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model, parts = _model(name), _parts(name)
    X, acq = J.one_member_inputs(name, kind, parts)
    eps = J.base_samples(4096, 1, 0)
    mu, var = A.moments(X[:, 0], *parts)
    terms = J.one_member_terms(acq, mu, var, eps)
    al = AGP.acquisition_joint(model, _py(AGP, acq), X, samples=4096, seed=0)  # the table of the seed
    assert A.relerr(al, terms.mean(axis=1)) <= PARITY
    se = terms.std(axis=1, ddof=1) / np.sqrt(4096)  # on the CPU, from the same table
    exact = AGP.acquisition(model, _py(AGP, acq), X[:, 0])  # the analytic EI / UCB on the device
    print(f"{kind}: {len(X)} points, largest |alpha - analytic| / se = {float(np.max(np.abs(al - exact) / se)):.2f}")
    assert len(X) >= 20 and np.all(se > 0) and np.all(np.abs(al - exact) <= 5 * se)


# ---- 4. the ascent --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", J.ASCENTS)
def test_ascent_against_the_restatement(env, name, T):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    X0, P, lo, hi, lr = J.ascent_inputs(name)
    eps = J.table(J.ASCENT_S, J.ASCENT_Q + 1)
    box = float(np.max(hi - lo))
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, np.minimum(np.maximum(X0, lo), hi), P, parts)
        wx, wa, margin = J.ascent(acq, X0, parts, eps, lo, hi, lr, T, P)
        gap = A.top_gap(wa)
        assert margin > J.KINK, (kind, minimize, margin)  # along the whole trajectory, on the device's own objects
        xb, ab, ib, X, Al = AGP.maximize_acquisition_joint(model, _py(AGP, acq), X0, (lo, hi), steps=T, lr=lr, full=True, **_kw(acq, P, eps))
        ex, ea = float(np.max(np.abs(X - wx)) / box), A.relerr(Al, wa)
        print(f"{name} T={T} {kind} minimize={minimize}: margin {margin:.1e} gap {gap:.1e};  device x {ex:.2e} of the box, alpha {ea:.2e}")
        assert X.shape == X0.shape and Al.shape == (len(X0),) and xb.shape == X0.shape[1:]
        assert ex <= PARITY and ea <= PARITY
        wi, wbx, wba = J.best(wx, wa)
        if gap > A.GAP:
            assert int(ib) == wi
            assert float(np.max(np.abs(xb - wbx)) / box) <= PARITY and abs(float(ab) - wba) <= PARITY * np.max(np.abs(wa))
        assert _same(xb, X[int(ib)]) and _same(ab, Al[int(ib)])
        x2, a2 = AGP.maximize_acquisition_joint(model, _py(AGP, acq), X0, (lo, hi), steps=T, lr=lr, **_kw(acq, P, eps))
        assert _same(x2, xb) and _same(a2, ab)


def test_zero_steps_and_pending_members(env):
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model, parts = _model(name), _parts(name)
    X0, P, lo, hi, lr = J.ascent_inputs(name)
    eps = J.table(J.ASCENT_S, J.ASCENT_Q + 1)
    acq = J.case_acq("ei", False, np.minimum(np.maximum(X0, lo), hi), P, parts)
    xb, ab, ib, X, Al = AGP.maximize_acquisition_joint(model, _py(AGP, acq), X0, (lo, hi), steps=0, lr=lr, full=True, **_kw(acq, P, eps))
    clipped = np.minimum(np.maximum(X0, lo), hi)
    assert np.array_equal(X, clipped) and X0[0, 0, 0] > hi[0]  # T = 0 returns the clipped starts
    wa, _, margin = J.alpha_grad(acq, clipped, parts, eps, P, grad=False)
    assert float(np.min(margin)) > J.KINK and A.relerr(Al, wa) <= PARITY
    wi, wbx, wba = J.best(X, Al)
    assert int(ib) == wi and _same(xb, wbx) and _same(ab, wba)
    # pending members are not in x_out (it holds the q optimised members only), the caller's array is untouched, and they matter: a
    # pending point changes the maximum only in the samples it wins, so this one stands next to the member with the best mean
    pts = clipped.reshape(-1, clipped.shape[2])
    P2 = pts[np.argmax(A.moments(pts, *parts)[0])][None] + 0.0125 * (hi - lo)
    Pd = env["torch"].as_tensor(P2, device="cuda")
    with_p = AGP.maximize_acquisition_joint(model, _py(AGP, acq), X0, (lo, hi), steps=5, lr=lr, full=True, base_samples=eps, pending=Pd)
    assert np.array_equal(Pd.cpu().numpy(), P2) and with_p[3].shape == X0.shape
    without = AGP.maximize_acquisition_joint(model, _py(AGP, acq), X0, (lo, hi), steps=5, lr=lr, full=True,
                                             base_samples=eps[:, :J.ASCENT_Q])
    assert not _same(with_p[3], without[3]) and A.relerr(with_p[4], without[4]) > 1e-6


# ---- 5. the bit-level contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d64-m64-r64"])
def test_bit_level_contract(env, name):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    model, parts = _model(name), _parts(name)
    X0, P, lo, hi, lr = J.ascent_inputs(name)
    R, q, D = X0.shape
    S, K = J.ASCENT_S, q + 1
    eps = J.table(S, K)
    acq = J.case_acq("ei", False, np.minimum(np.maximum(X0, lo), hi), P, parts)
    py, kw = _py(AGP, acq), _kw(acq, P, eps)
    Xt = A.data(name)["Xt"]
    before = (AGP.predict_f(model, Xt, cov=True), AGP.acquisition(model, py, Xt, grad=True))
    r1 = AGP.maximize_acquisition_joint(model, py, X0, (lo, hi), steps=5, lr=lr, full=True, **kw)
    r2 = AGP.maximize_acquisition_joint(model, py, X0, (lo, hi), steps=5, lr=lr, full=True, **kw)
    assert all(_same(a, b) for a, b in zip(r1, r2))  # a repeat
    perm = np.random.default_rng(5).permutation(R)
    r3 = AGP.maximize_acquisition_joint(model, py, X0[perm], (lo, hi), steps=5, lr=lr, full=True, **kw)
    assert _same(r3[3], r1[3][perm]) and _same(r3[4], r1[4][perm])  # a start does not see the others
    e1 = AGP.acquisition_joint(model, py, X0, grad=True, **kw)
    e3 = AGP.acquisition_joint(model, py, X0[perm], grad=True, **kw)
    assert _same(e3[0], e1[0][perm]) and _same(e3[1], e1[1][perm])
    # the handle is as it was
    h = model._ensure_handle(max(model._max_batch, 1))
    assert L.agp_svgp_check_status(h) == 0
    after = (AGP.predict_f(model, Xt, cov=True), AGP.acquisition(model, py, Xt, grad=True))
    assert all(_same(a, b) for pa, pb in zip(before, after) for a, b in zip(pa, pb))
    # pitched inputs and outputs, a padded lde: the same bits, the guard bands intact
    d = _desc(capi, acq)
    xin = Pitched("f64", data=X0.reshape(R * q, D), ld=D + 3, off=1, device="cuda")
    pin = Pitched("f64", data=P, ld=D + 2, off=1, device="cuda")
    ein = Pitched("f64", data=eps, ld=K + 3, off=1, device="cuda")
    oa = Pitched("f64", rows=1, width=R, off=1, device="cuda")
    og = Pitched("f64", rows=R * q, width=D, ld=D + 5, off=1, device="cuda")
    assert L.agp_svgp_acquisition_joint(h, 0, C.byref(d), _p(pin.ptr), D + 2, 1, q, _p(xin.ptr), D + 3, R, _p(ein.ptr), K + 3, S, _p(oa.ptr),
                                        _p(og.ptr), D + 5) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xin, "xq"), (pin, "xp"), (ein, "eps"), (oa, "alpha_out"), (og, "grad_out")):
        b.check(w)
    assert not oa.unwritten().any() and not og.unwritten().any()
    assert _same(oa.window()[0], e1[0]) and _same(og.window(), e1[1].reshape(R * q, D))
    opts, keep = _opts(capi, D, 5, lo, hi, lr)
    ox = Pitched("f64", rows=R * q, width=D, ld=D + 2, off=1, device="cuda")
    oA = Pitched("f64", rows=1, width=R, off=1, device="cuda")
    bx = Pitched("f64", rows=q, width=D, ld=D + 4, off=1, device="cuda")
    ba = Pitched("f64", rows=1, width=1, device="cuda")
    bi = Pitched("i64", rows=1, width=1, device="cuda")
    assert L.agp_svgp_acq_maximize_joint(h, 0, C.byref(d), _p(pin.ptr), D + 2, 1, q, _p(xin.ptr), D + 3, R, _p(ein.ptr), K + 3, S,
                                         C.byref(opts), _p(ox.ptr), D + 2, _p(oA.ptr), _p(bx.ptr), D + 4, _p(ba.ptr), _p(bi.ptr)) == 0
    L.agp_ctx_sync(model._ctx)
    for b, w in ((xin, "x0"), (pin, "xp"), (ein, "eps"), (ox, "x_out"), (oA, "a_out"), (bx, "best_x"), (ba, "best_a"), (bi, "best_idx")):
        b.check(w)
        assert b in (xin, pin, ein) or not b.unwritten().any(), w
    assert _same(ox.window(), r1[3].reshape(R * q, D)) and _same(oA.window()[0], r1[4]) and _same(bx.window(), r1[0])
    assert _same(ba.window()[0, 0], r1[1]) and int(bi.window()[0, 0]) == int(r1[2])
    ba2 = Pitched("f64", rows=1, width=1, device="cuda")  # any subset of the outputs
    assert L.agp_svgp_acq_maximize_joint(h, 0, C.byref(d), _p(pin.ptr), D + 2, 1, q, _p(xin.ptr), D + 3, R, _p(ein.ptr), K + 3, S,
                                         C.byref(opts), None, 0, None, None, 0, _p(ba2.ptr), None) == 0
    L.agp_ctx_sync(model._ctx)
    ba2.check("best_a alone")
    assert _same(ba2.window()[0, 0], r1[1])
    assert L.agp_svgp_check_status(h) == 0


def test_the_families_share_workspaces_without_disturbing_one_another(env):
    """The plain, greedy-batch and joint maximisers share the predictor's chunk workspaces, the particle state and the group sums on
    one handle.  Each of them called twice, with a joint evaluation (gradient included) between the two rounds, gives the same bits:
    nothing a call leaves behind reaches the next.  m = 65 (mp = 128), D = 3, 4097 starts -- two chunks of points, three of pairs --
    two steps, q = 2 with one pending point."""
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model = _model(name)
    D, spread, ctr = J._box(name)
    R, q, S = 4097, 2, 8
    rng = np.random.default_rng(20)
    X0 = ctr + spread * rng.uniform(-1.3, 1.3, size=(R, q, D))
    P = ctr + spread * rng.uniform(-1.3, 1.3, size=(1, D))
    lo, hi, lr = ctr - 2.0 * spread, ctr + 2.0 * spread, np.full(D, 0.03 * spread)
    eps = J.table(S, q + 1)
    py, kw = AGP.UCB(2.0), dict(steps=2, lr=lr, full=True)

    def round_():
        return (AGP.maximize_acquisition(model, py, X0[:, 0], (lo, hi), **kw),
                AGP.maximize_acquisition_batch(model, py, q, X0[:, 0], (lo, hi), pending=P, **kw),
                AGP.maximize_acquisition_joint(model, py, X0, (lo, hi), base_samples=eps, pending=P, **kw))

    first = round_()
    between = AGP.acquisition_joint(model, py, X0[:5], grad=True, base_samples=eps, pending=P)
    second = round_()
    assert first[0][3].shape == (R, D) and first[2][3].shape == (R, q, D) and np.all(np.isfinite(between[1]))
    for a, b in zip(first, second):
        assert len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))


# ---- 6. degenerate sets -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d1-m63-r63"])
def test_degenerate_sets(env, name):
    """two identical members, and a member on an inducing point: the jitter keeps C positive definite, so the factorisation succeeds.
    The yardstick's conditioning is stated in tests/test_acq_joint_host.py (test_conditioning_of_the_degenerate_sets): C has an
    eigenvalue of about the jitter, cond(C) ~ 4e4, and the gradient carries eps cond(C)^(3/2): compared within DEGENERATE_GRAD =
    2e-7, a hundred times the yardstick's own float64 rounding there; the values within PARITY."""
    AGP, L = env["AGP"], env["L"]
    model, parts = _model(name), _parts(name)
    X, P = J.degenerate(name)
    eps = J.table(64, 4, 5)
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, X, P, parts)
        wa, wg, margin = J.alpha_grad(acq, X, parts, eps, P)
        assert float(np.min(margin)) > J.KINK
        al, g = AGP.acquisition_joint(model, _py(AGP, acq), X, grad=True, **_kw(acq, P, eps))
        ea, eg = A.relerr(al, wa), A.relerr(g, wg)
        print(f"{name} {kind} minimize={minimize}: alpha {ea:.2e}  grad {eg:.2e}")
        assert np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        assert ea <= PARITY and eg <= DEGENERATE_GRAD
    assert L.agp_svgp_check_status(model._ensure_handle(max(model._max_batch, 1))) == 0


# ---- 7. refusals and argument checks ----------------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_argument_checks(env):
    AGP, L, capi, torch = env["AGP"], env["L"], env["capi"], env["torch"]
    rng = np.random.default_rng(0)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    names = ("agp_svgp_acquisition_joint", "agp_svgp_acq_maximize_joint")

    def sparse(kernel, D, T=np.float64):
        X = rng.standard_normal((40, D))
        y = np.where(X[:, 0] > 0, 1, -1)
        m = AGP.SVGP(kernel, AGP.LogisticLikelihood(), AGP.AnalyticSVI(20), X[:6].copy(), optimiser=False, T=T)
        AGP.train_(m, X, y, 2)
        return m, X

    def both(model, X, desc, opts, latent=0, n=1, q=2, S=8, lde=None, ldp=None, ldx=None, ldg=None, ldb=None, xp_null=False, x_null=False,
             eps_null=False, who=names):
        """(status, message) of the two entry points on 4 tuples of q points; asserts that every output stayed NaN"""
        m = _svgp(model)
        h = m._ensure_handle(max(m._max_batch, 1))
        D = X.shape[1]
        qa, na = max(q, 1), max(n, 1)
        Xd = torch.as_tensor(X[:4 * qa], dtype=torch.float64, device="cuda").contiguous()
        Pd = torch.as_tensor(X[-na:], dtype=torch.float64, device="cuda").contiguous()
        E = torch.zeros(4100, 20, dtype=torch.float64, device="cuda")
        outs = [nan(4), nan(4 * qa, D), nan(4 * qa, D), nan(4), nan(qa, D), nan(1)]
        bi = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        xp, xq, ep = (None if xp_null else _p(Pd.data_ptr())), (None if x_null else _p(Xd.data_ptr())), (None if eps_null else _p(E.data_ptr()))
        ldp_, ldx_, lde_ = (D if ldp is None else ldp), (D if ldx is None else ldx), (20 if lde is None else lde)
        res = []
        if names[0] in who:
            st = L.agp_svgp_acquisition_joint(h, latent, desc, xp, ldp_, n, q, xq, ldx_, 4, ep, lde_, S, _p(outs[0].data_ptr()),
                                              _p(outs[1].data_ptr()), D if ldg is None else ldg)
            res.append((st, L.agp_last_error(m._ctx).decode()))
        if names[1] in who:
            st = L.agp_svgp_acq_maximize_joint(h, latent, desc, xp, ldp_, n, q, xq, ldx_, 4, ep, lde_, S, opts, _p(outs[2].data_ptr()),
                                               D if ldg is None else ldg, _p(outs[3].data_ptr()), _p(outs[4].data_ptr()),
                                               D if ldb is None else ldb, _p(outs[5].data_ptr()), _p(bi.data_ptr()))
            res.append((st, L.agp_last_error(m._ctx).decode()))
        L.agp_ctx_sync(m._ctx)
        assert all(bool(torch.isnan(o).all()) for o in outs) and int(bi[0]) == -7
        return res

    def expect(res, status, text, who=names):
        assert len(res) == len(who)
        for (st, msg), w in zip(res, who):
            assert st == status and w in msg and text in msg, (st, msg, w, text)

    good = capi.AcqDesc(1, 0, 0.0, 0.1, 0.01)
    X2 = rng.standard_normal((40, 2))
    mc = AGP.MCGP(X2, np.where(X2[:, 0] > 0, 1, -1), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    unsupported = [("AGP_F32", ) + sparse(AGP.SqExponentialKernel(), 3, T=np.float32),
                   ("ExponentialKernel", ) + sparse(AGP.ExponentialKernel(), 3),
                   ("at most 64", ) + sparse(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.2), 65),
                   ("AGP_FLAG_SAMPLED", mc, X2),
                   ("multi-output", _model_mo(AGP), rng.standard_normal((40, 3)))]
    for text, model, X in unsupported:
        opts, keep = _opts(capi, X.shape[1], 3, -1.0, 1.0, 0.1)
        expect(both(model, X, C.byref(good), C.byref(opts)), UNSUPPORTED, text)
    model, X = sparse(AGP.Matern32Kernel(), 3)
    opts, keep = _opts(capi, 3, 3, -1.0, 1.0, 0.1)
    ok = C.byref(opts)
    for kind, text in ((2, "AGP_ACQ_PI"), (5, "AGP_ACQ_LOG_EI"), (6, "AGP_ACQ_LOG_PI")):
        expect(both(model, X, C.byref(capi.AcqDesc(kind, 0, 0.0, 0.1, 0.0)), ok), UNSUPPORTED, text + " has no joint form")
    expect(both(model, X, None, ok), INVALID, "desc must be given")
    for bad, text in ((capi.AcqDesc(3, 0, 0.0, 0.0, 0.0), "unknown kind"), (capi.AcqDesc(0, 0, -1.0, 0.0, 0.0), "beta >= 0"),
                      (capi.AcqDesc(1, 0, 0.0, 0.0, -0.5), "xi >= 0"), (capi.AcqDesc(1, 0, 0.0, float("inf"), 0.0), "finite")):
        expect(both(model, X, C.byref(bad), ok), INVALID, text)
    g = C.byref(good)
    expect(both(model, X, g, ok, latent=1), INVALID, "latent")
    expect(both(model, X, g, ok, q=0), INVALID, "q >= 1")
    expect(both(model, X, g, ok, n=-1), INVALID, "n_pending >= 0")
    expect(both(model, X, g, ok, q=2, n=15), INVALID, "AGP_ACQ_JOINT_MAX_Q")  # q + n = 17
    expect(both(model, X, g, ok, q=17, n=0), INVALID, "AGP_ACQ_JOINT_MAX_Q")
    expect(both(model, X, g, ok, S=0), INVALID, "[1, 4096]")
    expect(both(model, X, g, ok, S=4097), INVALID, "[1, 4096]")
    expect(both(model, X, g, ok, eps_null=True), INVALID, "eps must be given")
    expect(both(model, X, g, ok, lde=2), INVALID, "lde >= q + n_pending")
    expect(both(model, X, g, ok, xp_null=True), INVALID, "xp must be given")
    expect(both(model, X, g, ok, ldp=2), INVALID, "ldp >= D")
    expect(both(model, X, g, ok, ldx=2), INVALID, "ld")
    expect(both(model, X, g, ok, ldg=2), INVALID, "ld")
    expect(both(model, X, g, ok, x_null=True, who=names[:1]), INVALID, "NULL", names[:1])
    mx = names[1:]
    expect(both(model, X, g, ok, x_null=True, who=mx), INVALID, "x0 must be given", mx)
    expect(both(model, X, g, ok, ldb=2, who=mx), INVALID, "ldb >= D", mx)
    expect(both(model, X, g, None, who=mx), INVALID, "opts must be given", mx)
    for kw, text in ((dict(steps=-1), "steps"), (dict(beta1=1.0), "beta1"), (dict(eps=0.0), "eps"), (dict(lo=1.0, hi=-1.0), "lo <= hi"),
                     (dict(lr=0.0), "step sizes"), (dict(minimize=1), "opts->minimize")):
        a = dict(steps=3, lo=-1.0, hi=1.0, lr=0.1)
        a.update(kw)
        o, keep = _opts(capi, 3, a.pop("steps"), a.pop("lo"), a.pop("hi"), a.pop("lr"), **a)
        expect(both(model, X, g, C.byref(o), who=mx), INVALID, text, mx)
    h = model._ensure_handle(max(model._max_batch, 1))
    Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda").contiguous()
    E = torch.zeros(8, 2, dtype=torch.float64, device="cuda")
    assert L.agp_svgp_acq_maximize_joint(h, 0, g, None, 3, 0, 2, _p(Xd.data_ptr()), 3, 4, _p(E.data_ptr()), 2, 8, ok, None, 3, None, None, 3,
                                         None, None) == INVALID
    assert "at least one output" in L.agp_last_error(model._ctx).decode()
    assert L.agp_svgp_acq_maximize_joint(h, 0, g, None, 3, 0, 2, _p(Xd.data_ptr()), 3, 0, _p(E.data_ptr()), 2, 8, ok, None, 3, None, None, 3,
                                         _p(Xd.data_ptr()), None) == INVALID
    assert "n_starts" in L.agp_last_error(model._ctx).decode()
    # n_sets = 0 is a successful no-op, n_pending = 0 does not look at xp, and the handle still works
    out = nan(4)
    assert L.agp_svgp_acquisition_joint(h, 0, g, None, 0, 0, 2, _p(Xd.data_ptr()), 3, 0, _p(E.data_ptr()), 2, 8, _p(out.data_ptr()), None, 3) == 0
    L.agp_ctx_sync(model._ctx)
    assert bool(torch.isnan(out).all())
    assert L.agp_svgp_acquisition_joint(h, 0, g, None, 0, 0, 2, _p(Xd.data_ptr()), 3, 4, _p(E.data_ptr()), 2, 8, _p(out.data_ptr()), None, 3) == 0
    L.agp_ctx_sync(model._ctx)
    assert not bool(torch.isnan(out).any()) and L.agp_svgp_check_status(h) == 0


def test_python_refusals_on_the_device(env):
    """the mirror refuses before the device is touched: with a trained model at hand the same errors, and nothing has run"""
    AGP = env["AGP"]
    model = _model("m65-logistic-m32-ard")
    X = np.zeros((4, 2, 3))
    for acq in (AGP.PI(0.0), AGP.LogEI(0.0), AGP.LogPI(0.0)):
        with pytest.raises(NotImplementedError, match="has no joint form"):
            AGP.acquisition_joint(model, acq, X)
        with pytest.raises(NotImplementedError, match="has no joint form"):
            AGP.maximize_acquisition_joint(model, acq, X, (-1.0, 1.0))
    with pytest.raises(NotImplementedError, match="multi-output"):
        AGP.acquisition_joint(_model_mo(AGP), AGP.UCB(), X)
    for kw, match in ((dict(pending=np.zeros((15, 3))), "exceed 16"), (dict(samples=0), r"\[1, 4096\]"), (dict(samples=4097), r"\[1, 4096\]"),
                      (dict(base_samples=np.zeros((8, 3))), "base_samples must be")):
        with pytest.raises(ValueError, match=match):
            AGP.acquisition_joint(model, AGP.UCB(), X, **kw)
    with pytest.raises(ValueError, match="Xq must be"):
        AGP.acquisition_joint(model, AGP.UCB(), np.zeros((4, 2, 2)))
    with pytest.raises(ValueError, match="X0 must be"):
        AGP.maximize_acquisition_joint(model, AGP.UCB(), np.zeros((4, 3)), (-1.0, 1.0))
