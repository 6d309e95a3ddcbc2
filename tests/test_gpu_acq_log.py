"""LogEI and LogPI on the MI355X (include/agp_hip.h, "ACQUISITION FUNCTIONS"; csrc/agp_acq_log.h): agp_acq_moments against mpmath
on the grid of tests/_acq_log_ref.py, agp_svgp_acquisition, agp_svgp_acq_maximize, the pending path and the batch rounds against the
NumPy restatement fed with the DEVICE's own predictor objects, where EI and PI are exactly 0 with a zero gradient -- the defect the
log kinds are there for --, the limits, the plain kinds' bits before and after log-kind calls on the same handle, and the ABI.

The measure: |got - want| <= PARITY max(1, |want|) for log alpha and |got - want| <= PARITY |want| for the point function's two
derivatives; a gradient in x, a sum of two products that may cancel, is compared as the plain kinds' is: max |got - want| <= PARITY
max |want| (_acq_ref.relerr).  PARITY = 1e-8 is the project's parity bound; COND_CAP and GAP are those of the pathwise ascent.
The shapes are the smallest at which this code can go wrong: m = 63, 65 and 130 lie off the contraction's 32-column tiles, D is 1
and 3, n_t = 130 crosses the 64-particle workgroup twice and leaves a tail of 2.
"""
import ctypes as C

import numpy as np
import pytest

import _acq_log_ref as LR
import _acq_ref as A
import _predgrad_cases as PC
from test_acq_log_host import _limit_cases, _limits_want, assert_point
from test_gpu_acq import INVALID, _model, _p, _parts, _same

pytestmark = pytest.mark.gpu

PARITY = A.PARITY
EPS = float(np.finfo(np.float64).eps)
OFF_TILE = ["d1-m63-r63", "m65-logistic-m32-ard", "gp", "m130-d3-r4133"]  # m = 63, 65, 65 (exact GP), 130; D = 1, 3, 3, 3


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi

    return dict(AGP=AGP, capi=capi, L=capi.lib(), torch=torch)


def _py(AGP, q):
    cls = {"ucb": AGP.UCB, "ei": AGP.EI, "pi": AGP.PI, "logei": AGP.LogEI, "logpi": AGP.LogPI}[q["kind"]]
    return cls(q["beta"]) if q["kind"] == "ucb" else cls(q["best"], q["xi"])


# ---- 1. the point function on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_moments_against_mpmath(env, kind, minimize):
    AGP = env["AGP"]
    s = -1.0 if minimize else 1.0
    mu, var = LR.grid_moments(s)
    acq = _py(AGP, LR.acq(kind))
    al, dm, dv = AGP.acquisition_moments(acq, mu, var, minimize=minimize, grad=True)
    assert_point((al, dm, dv * 2 * np.sqrt(var)), LR.mp_grid(kind, s), f"device {kind} s={s:+.0f} against mpmath")
    assert _same(AGP.acquisition_moments(acq, mu, var, minimize=minimize), al)  # the derivatives are optional: the same bits


def test_the_off_tile_cases_are_off_the_tiles():
    sp = [A.spec(n) for n in OFF_TILE]
    assert [c["m"] for c in sp] == [63, 65, 65, 130] and all(c["m"] % 32 for c in sp) and [c["D"] for c in sp] == [1, 3, 3, 3]


# ---- 2. acquisition(..., grad=True) where the plain kinds are zero ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", OFF_TILE)
def test_acquisition_where_ei_and_pi_are_zero(env, name):
    AGP = env["AGP"]
    model, parts = _model(name), _parts(name)
    Xt = A.data(name)["Xt"][:130]
    assert len(Xt) == 130
    mu, var = A.moments(Xt, *parts)
    best = float(np.max(mu)) + 60.0 * float(np.sqrt(parts[2] + A.JITTER))  # 60 prior standard deviations above the largest mean
    assert np.all((mu - best - A.XI) / np.sqrt(var) <= -60.0)
    for plain, kind in (("ei", "logei"), ("pi", "logpi")):
        pa, pg = AGP.acquisition(model, _py(AGP, A.acq(plain, best=best, xi=A.XI)), Xt, grad=True)
        assert pa.shape == (130,) and pg.shape == Xt.shape and np.all(pa == 0.0) and np.all(pg == 0.0)  # the defect
        q = LR.acq(kind, best=best, xi=A.XI)
        al, g = AGP.acquisition(model, _py(AGP, q), Xt, grad=True)
        wa, wg, _, _ = LR.alpha_grad(q, Xt, parts)
        ea, eg = float(LR.err_alpha(al, wa).max()), A.relerr(g, wg)
        print(f"{name} {kind}: log alpha in [{al.min():.1f}, {al.max():.1f}]  error {ea:.2e}  gradient {eg:.2e}")
        assert al.shape == (130,) and g.shape == Xt.shape and np.all(np.isfinite(al)) and np.all(np.isfinite(g))
        assert np.all(np.any(g != 0.0, axis=1))
        assert ea <= PARITY and eg <= PARITY
        assert _same(AGP.acquisition(model, _py(AGP, q), Xt), al)  # values only: the same bits


# ---- 3. the limits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LR.KINDS)
def test_moments_zero_variance_and_nan(env, kind):
    """exact, but for log imp of LogEI, which is the device's log against NumPy's: two units of the last place; with imp = 1 it is 0"""
    AGP = env["AGP"]
    for minimize in (False, True):
        s = -1.0 if minimize else 1.0
        acq = _py(AGP, LR.acq(kind, best=0.5))
        for mu4, var4 in _limit_cases():
            mu = np.concatenate([mu4, [0.5 + s, np.nan, 0.3, np.nan]])  # (imp = 1 at index 4)
            var = np.concatenate([var4, [var4[0], 1.0, np.nan, var4[0]]])
            al, dm, dv = AGP.acquisition_moments(acq, mu, var, minimize=minimize, grad=True)
            wa, wm = _limits_want(kind, s, mu4)
            assert np.all(np.isnan(al[5:])) and np.all(np.isnan(dm[5:])) and np.all(np.isnan(dv[5:]))
            assert np.array_equal(dm[:4], wm) and np.all(dv[:5] == 0.0) and np.array_equal(np.isneginf(al[:4]), np.isneginf(wa))
            fin = np.isfinite(wa)
            assert np.all(np.abs(al[:4][fin] - wa[fin]) <= 2 * EPS * np.abs(wa[fin]))
            assert al[4] == 0.0 and dm[4] == (s if kind == "logei" else 0.0)
            assert _same(AGP.acquisition_moments(acq, mu, var, minimize=minimize), al)


# ---- 4. the plateau -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plateau(env):
    model = LR.plateau_model(env["AGP"])
    return model, LR.device_parts(model)


@pytest.mark.parametrize("plain,kind", LR.PLATEAU_KINDS)
def test_plateau(env, plateau, plain, kind):
    AGP = env["AGP"]
    model, parts = plateau
    assert model.m == 40 and model.D == 1
    X0, lo, hi, lr = LR.plateau_inputs()
    T = LR.PLATEAU["T"]
    best = LR.plateau_best(parts, X0, lo, hi)
    x0 = np.minimum(np.maximum(X0, lo), hi)
    # the plain kind: nothing moves, and the best-start rule picks among equal zeros
    _, pab, pib, pX, pA = AGP.maximize_acquisition(model, _py(AGP, A.acq(plain, best=best)), X0, (lo, hi), steps=T, lr=lr, full=True)
    assert _same(pX, x0) and np.all(pA == 0.0) and float(pab) == 0.0 and int(pib) == 0
    # the log kind: conditioned on the device's own objects, then within PARITY of the restatement
    q = LR.acq(kind, best=best)
    wx, wa = LR.ascent(q, X0, parts, lo, hi, lr, T)
    lx, la = LR.ascent(q, X0, parts, lo, hi, lr, T, dtype=np.longdouble)
    box = float(np.max(hi - lo))
    cx, ca, gap = float(np.max(np.abs(wx - lx)) / box), A.relerr(wa, la), A.top_gap(wa)
    assert cx <= A.COND_CAP and ca <= A.COND_CAP, (cx, ca)
    assert gap > A.GAP, gap  # (the inputs were chosen so that the index is compared: tests/test_acq_log_host.py)
    xb, ab, ib, X, Al = AGP.maximize_acquisition(model, _py(AGP, q), X0, (lo, hi), steps=T, lr=lr, full=True)
    ex, ea = float(np.max(np.abs(X - wx)) / box), float(LR.err_alpha(Al, wa).max())
    print(f"{kind}: conditioning x {cx:.1e} log alpha {ca:.1e} gap {gap:.1e};  device x {ex:.2e} of the box, log alpha {ea:.2e}")
    assert np.all(np.isfinite(Al)) and ex <= PARITY and ea <= PARITY
    a0 = AGP.acquisition(model, _py(AGP, q), x0)
    assert np.all(np.isfinite(a0)) and np.all(Al > a0) and not np.any(X == x0)  # every start climbs
    wi, wbx, wba = A.best(wx, wa)
    assert int(ib) == wi and _same(xb, X[wi]) and _same(ab, Al[wi])
    assert np.all(X >= lo) and np.all(X <= hi) and X0[0, 0] > hi[0]


# ---- 5. pending points and batches --------------------------------------------------------------------------------------------------------------
def _pending_inputs(name):
    """(P (3, D), X: six points within 1e-3 of P[1] and seven of the case's test points)"""
    Xt = A.data(name)["Xt"]
    P = Xt[:3].copy()
    rng = np.random.default_rng(1)
    U = rng.standard_normal((6, P.shape[1]))
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    X = np.vstack([P[1] + 1e-3 * rng.uniform(0.1, 1.0, (6, 1)) * U, Xt[3:10]])
    assert np.all(np.linalg.norm(X[:6] - P[1], axis=1) <= 1e-3)
    return P, X


@pytest.mark.parametrize("kind", LR.KINDS)
def test_pending(env, kind):
    AGP = env["AGP"]
    name = "gp"
    model, parts = _model(name), _parts(name)
    P, X = _pending_inputs(name)
    best = float(np.max(A.moments(A.data(name)["Xt"], *parts)[0]))
    q = LR.acq(kind, best=best, xi=A.XI)
    wa, wg, mu, var = LR.alpha_grad(q, X, parts, pending=P, tau2=0.0)
    ld = LR.alpha_grad(q, X, parts, pending=P, tau2=0.0, dtype=np.longdouble)
    z = (mu - best - A.XI) / np.sqrt(var)
    assert np.all(z[:6] < -38.0) and np.any(z[6:] > LR.BRANCH)  # next to the pending point EI and PI have underflowed
    assert float(LR.err_alpha(wa, ld[0]).max()) <= 1e-10 and A.relerr(wg, ld[1]) <= 1e-10  # the restatement is conditioned there
    al, g = AGP.acquisition(model, _py(AGP, q), X, grad=True, pending=P)
    ea, eg = float(LR.err_alpha(al, wa).max()), A.relerr(g, wg)
    print(f"{kind} with 3 pending points: z in [{z.min():.1f}, {z.max():.1f}]  log alpha {ea:.2e}  gradient {eg:.2e}")
    assert np.all(np.isfinite(al)) and np.all(np.isfinite(g)) and ea <= PARITY and eg <= PARITY
    pa = AGP.acquisition(model, _py(AGP, A.acq(LR.PLAIN[kind], best=best, xi=A.XI)), X, pending=P)
    assert np.all(pa[:6] == 0.0) and np.all(pa[6:] > 0.0)
    assert _same(AGP.acquisition(model, _py(AGP, q), X, pending=P), al)


def test_batch_equals_chained_calls(env):
    AGP = env["AGP"]
    name = "gp"
    model, parts = _model(name), _parts(name)
    X0, lo, hi, lr = A.inputs(name)
    acq = _py(AGP, LR.acq("logei", best=float(np.max(A.moments(np.minimum(np.maximum(X0, lo), hi), *parts)[0])), xi=A.XI))
    Xb, ab, ib = AGP.maximize_acquisition_batch(model, acq, 3, X0, (lo, hi), steps=20, lr=lr, full=True)
    assert Xb.shape == (3, X0.shape[1]) and np.all(np.isfinite(ab)) and len({tuple(x) for x in Xb}) == 3
    won = None
    for b in range(3):
        x1, a1, i1 = AGP.maximize_acquisition_batch(model, acq, 1, X0, (lo, hi), steps=20, lr=lr, full=True, pending=won)
        assert _same(x1[0], Xb[b]) and _same(a1[0], ab[b]) and int(i1[0]) == int(ib[b]), b
        won = x1 if won is None else np.vstack([won, x1])
    x, a, i, _, _ = AGP.maximize_acquisition(model, acq, X0, (lo, hi), steps=20, lr=lr, full=True)
    assert _same(x, Xb[0]) and _same(a, ab[0]) and int(i) == int(ib[0])  # no pending point, q = 1: agp_svgp_acq_maximize


# ---- 6. the plain kinds keep their bits ---------------------------------------------------------------------------------------------------------
def test_plain_kinds_unchanged_by_log_kind_calls(env):
    """one handle: UCB, EI, PI before any log-kind call, every log-kind path, then the same calls again -- nothing leaks through the
    particle state or the pending workspaces"""
    AGP = env["AGP"]
    name = "m65-logistic-m32-ard"
    model = PC.make_model(AGP, A.CASES[name]["pc"])  # a handle that has seen no acquisition call
    Xt = A.data(name)["Xt"][:130]
    X0, lo, hi, lr = A.inputs(name)
    best = 0.2
    plain = [AGP.UCB(2.0), AGP.EI(best, A.XI), AGP.PI(best, A.XI)]

    def run():
        out = []
        for acq in plain:
            out += list(AGP.acquisition(model, acq, Xt, grad=True))
            out += list(AGP.maximize_acquisition(model, acq, X0, (lo, hi), steps=5, lr=lr, full=True))
            out += list(AGP.maximize_acquisition_batch(model, acq, 2, X0, (lo, hi), steps=3, lr=lr, pending=Xt[:2]))
        return out

    before = run()
    for acq in (AGP.LogEI(best, A.XI), AGP.LogPI(best, A.XI), AGP.LogEI(best + 100.0), AGP.LogPI(best + 100.0)):
        AGP.acquisition(model, acq, Xt, grad=True)
        AGP.acquisition(model, acq, Xt, pending=Xt[:3])
        AGP.maximize_acquisition(model, acq, np.vstack([X0, X0[:7]]), (lo, hi), steps=5, lr=lr)  # (more starts: the state grows)
        AGP.maximize_acquisition_batch(model, acq, 3, X0, (lo, hi), steps=3, lr=lr)
    after = run()
    assert len(before) == len(after) == 27 and all(_same(a, b) for a, b in zip(before, after))


# ---- 7. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_kinds(env):
    L, capi, torch = env["L"], env["capi"], env["torch"]
    name = "m65-logistic-m32-ard"
    model = _model(name)
    ctx = model._ctx
    h = model._ensure_handle(max(model._max_batch, 1))
    Xd = torch.as_tensor(A.data(name)["Xt"][:8], dtype=torch.float64, device="cuda").contiguous()
    mu, var = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.ones(8, dtype=torch.float64, device="cuda")
    nan = lambda: torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")

    def both(desc):
        """(status, message, output) of agp_acq_moments and of agp_svgp_acquisition"""
        res = []
        for call in (lambda o: L.agp_acq_moments(ctx, C.byref(desc), 8, _p(mu.data_ptr()), _p(var.data_ptr()), _p(o.data_ptr()), None, None),
                     lambda o: L.agp_svgp_acquisition(h, 0, C.byref(desc), _p(Xd.data_ptr()), 3, 8, _p(o.data_ptr()), None, 3)):
            out = nan()
            st = call(out)
            msg = L.agp_last_error(ctx).decode()
            L.agp_ctx_sync(ctx)
            res.append((st, msg, out.cpu().numpy()))
        return res

    assert (capi.ACQ_LOG_EI, capi.ACQ_LOG_PI) == (5, 6)
    for kind in (5, 6):
        for st, _, out in both(capi.AcqDesc(kind, 0, 0.0, 0.1, 0.01)) + both(capi.AcqDesc(kind, 1, 0.0, 0.1, 0.0)):
            assert st == 0 and np.all(np.isfinite(out))
        for bad, text in ((capi.AcqDesc(kind, 0, 0.0, 0.1, -0.5), "xi >= 0"), (capi.AcqDesc(kind, 0, 0.0, float("inf"), 0.0), "finite"),
                          (capi.AcqDesc(kind, 0, 0.0, 0.1, float("nan")), "finite")):
            for st, msg, out in both(bad):
                assert st == INVALID and text in msg and np.all(np.isnan(out)), (kind, st, msg)
    for kind in (3, 4, 7, 8, -1):
        for (st, msg, out), who in zip(both(capi.AcqDesc(kind, 0, 0.0, 0.1, 0.01)), ("agp_acq_moments", "agp_svgp_acquisition")):
            assert st == INVALID and "unknown kind" in msg and who in msg and np.all(np.isnan(out)), (kind, st, msg)
