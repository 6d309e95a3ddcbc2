"""CPU tests of batch acquisition with pending points (include/agp_hip.h, "ACQUISITION FUNCTIONS", paragraph "Pending points"): the
three forms of the conditioned variance agree (direct Schur form, augmented predictor by blocks, augmented predictor by bordering), the
refit identity of the exact GP, the conditioning of every input the GPU suite compares (on the oracle's objects: float64 against long
double, 100 times below PARITY, so that rounding in the yardstick cannot decide a GPU test), and the host mirror's argument checks.
"""
import os
import re

import numpy as np
import pytest

import _acq_batch_ref as B
import _acq_ref as A
import _predgrad_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK = 1e-10  # float64 against long double of the restatement: PARITY / 100


def _close(a, b):
    return A.relerr(a, b)


# ---- 1, 2. the three forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gp", "m65-logistic-m32-ard", "m1-r1", "d64-m64-r64"])
@pytest.mark.parametrize("tau2", B.NOISES)
def test_augmented_form_equals_direct_form(name, tau2):
    """in long double, where the three can be told apart from rounding: direct == blocks == bordering"""
    parts, P, X = A.oracle_parts(name), B.pending(name), B.eval_points(name)[:80]
    ld = np.longdouble
    _, var_d, _, _ = B.moments_grads(X, parts, P, tau2, dtype=ld)
    Zb, ab, Ab = B.augmented(parts, P, tau2, dtype=ld)
    Zo, ao, Ao, cs = B.border(parts, P, tau2, dtype=ld)
    var_b, var_o = B.var_augmented(X, parts, Zb, Ab, dtype=ld), B.var_augmented(X, parts, Zo, Ao, dtype=ld)
    scale = float(np.max(np.abs(var_d)))
    eb, eo = float(np.max(np.abs(var_b - var_d))) / scale, float(np.max(np.abs(var_o - var_d))) / scale
    eA = _close(Ao, Ab)
    print(f"{name} tau2={tau2}: n = {len(P)}  blocks {eb:.2e}  bordering {eo:.2e}  A' bordering against blocks {eA:.2e}  min c {float(min(cs)):.3e}")
    # k'' A' k' is a sum of (m + n)^2 products of size |A'| v^2 that cancels to (v + jitter) - var_P: in long double (eps 1.1e-19) its
    # absolute error is about eps (m + n) max|A'| v^2, taken relative to the largest variance, with a factor 16 for the constant; the
    # entries of A' themselves carry eps (m + n) max|A'| (v + jitter + tau2) relative, with a factor 64 (two routes, n steps)
    eps, mn, v = float(np.finfo(ld).eps), len(parts[0]) + len(P), float(parts[2])
    amax = float(np.max(np.abs(Ab)))
    assert eb <= 16 * eps * mn * amax * v * v / scale and eo <= 16 * eps * mn * amax * v * v / scale
    assert eA <= 64 * eps * mn * amax * (v + B.JITTER + tau2)
    assert np.array_equal(Zb, Zo) and np.array_equal(ab, ao) and not np.any(ab[len(parts[0]):])
    assert all(c > 0 for c in cs) and Ao.shape == (len(parts[0]) + len(P),) * 2
    # the mean is untouched: a' = [a; 0]
    k = parts[2] * G.phi(parts[3], G.sqdist(X, Zo.astype(np.float64), np.broadcast_to(np.asarray(parts[1], dtype=np.float64), (X.shape[1],))))
    assert _close(k @ ao.astype(np.float64), A.moments(X, *parts)[0]) <= 1e-14


def test_bordering_one_by_one_is_the_bordering_of_the_whole_set():
    """a pending set passed in and a set accumulated point by point: the same operations, the same bits"""
    name = "m65-logistic-m32-ard"
    parts, P = A.oracle_parts(name), B.pending(name)
    Z1, a1, A1, _ = B.border(parts, P, 0.01)
    Zs, as_, As, _ = B.border(parts, P[:2], 0.01)
    for p in P[2:]:
        Zs, as_, As, _ = B.border((Zs, parts[1], parts[2], parts[3], as_, As), p[None], 0.01)
    assert np.array_equal(A1, As) and np.array_equal(Z1, Zs)


# ---- 3. the refit identity ------------------------------------------------------------------------------------------------------------------
def test_refit_identity():
    """exact GP with noise sigma^2, tau2 = sigma^2: conditioning on mu(P) at P is the GP refitted on (X u P, y u mu(P)) with the same
    hyper-parameters.  The GP's A is (K + jitter I + sigma^2 I)^-1, so the refitted one carries jitter + sigma^2 on the diagonal of
    the pending block: the C of the header."""
    name, noise = "gp", 0.05
    parts, P, Xt = A.oracle_parts(name), B.pending(name), B.eval_points(name)
    Z, s, v, kind, a, Ap = parts
    sc = np.broadcast_to(np.asarray(s, dtype=np.float64), (Z.shape[1],))
    y = np.linalg.solve(Ap, a)
    assert _close(np.linalg.inv(Ap), v * G.phi(kind, G.sqdist(Z, Z, sc)) + (noise + B.JITTER) * np.eye(len(Z))) <= 1e-10  # (it is that GP)
    muP = A.moments(P, *parts)[0]
    X2, y2 = np.vstack([Z, P]), np.concatenate([y, muP])
    K2 = v * G.phi(kind, G.sqdist(X2, X2, sc)) + (noise + B.JITTER) * np.eye(len(X2))
    ks = v * G.phi(kind, G.sqdist(Xt, X2, sc))
    mu2 = ks @ np.linalg.solve(K2, y2)
    var2 = v + B.JITTER - np.sum(ks * np.linalg.solve(K2, ks.T).T, axis=1)
    mu, var, _, _ = B.moments_grads(Xt, parts, P, noise)
    em, ev = _close(mu, mu2), _close(var, var2)
    print(f"refit: mean {em:.2e}  variance {ev:.2e}")
    assert em <= 1e-10 and ev <= 1e-10


# ---- 4. the yardstick of the parity tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.PENDING))
@pytest.mark.parametrize("tau2", B.NOISES)
def test_yardstick_of_the_parity_inputs(name, tau2):
    parts, P, X = A.oracle_parts(name), B.pending(name), B.eval_points(name)
    if len(X) > 600:  # the chunk case: the first and the last points and the pending ones (long double over 4133 x 130 three times)
        X = np.vstack([X[:200], X[-200:]])
    X0, lo, hi, _ = A.inputs(name)
    for kind in A.KINDS:
        q = A.case_acq(kind, X0, parts, lo, hi)
        a64, g64, _, v64 = B.alpha_grad(q, X, parts, P, tau2)
        ald, gld, _, vld = B.alpha_grad(q, X, parts, P, tau2, dtype=np.longdouble)
        ea, eg, ev = _close(a64, ald), _close(g64, gld), _close(v64, vld)
        print(f"{name} {kind} tau2={tau2}: alpha {ea:.2e}  grad {eg:.2e}  var_P {ev:.2e}")
        assert ea <= YARDSTICK and eg <= YARDSTICK and ev <= YARDSTICK


def test_pending_sets_have_their_edges():
    for name, n in B.PENDING.items():
        P, c = B.pending(name), A.spec(name)
        assert P.shape == (n, c["D"])
        if n >= 2:
            assert np.array_equal(P[n - 1], P[n // 2])
        if c["kind"] != "sqexponential":
            d = A.data(name)
            assert np.array_equal(P[0], (d["Z"] if "Z" in d else d["X"])[0])
    mp = {(A.spec(n)["m"], k) for n, k in B.PENDING.items()}
    assert {(63, 1), (64, 1), (1, 63), (65, 5), (130, 5)} <= mp  # m' = 64, 65, 64, 70, 135


# ---- 5. the conditioning of the batches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.BATCHES, ids=B.batch_id)
def test_conditioning_of_the_batches(case):
    name, kind, tau2, npend, nq, T = case
    parts = A.oracle_parts(name)
    X0, lo, hi, lr = A.inputs(name)
    q = A.case_acq(kind, X0, parts, lo, hi)
    P = B.pending(name, npend) if npend else np.zeros((0, X0.shape[1]))
    r64 = B.batch(q, nq, X0, parts, P, tau2, lo, hi, lr, T)
    rld = B.batch(q, nq, X0, parts, P, tau2, lo, hi, lr, T, dtype=np.longdouble)
    ex, ea, gap, same = B.conditioning(r64, rld, lo, hi)
    print(f"{B.batch_id(case)}: x {ex:.2e} of the box, alpha {ea:.2e}, smallest top gap {gap:.2e}, indices {[r['idx'] for r in r64]}")
    assert ex <= A.COND_CAP and ea <= A.COND_CAP
    assert gap > A.GAP
    assert same
    xs = np.array([r["x"] for r in r64])
    assert np.all(xs >= lo) and np.all(xs <= hi)


# ---- the host mirror ------------------------------------------------------------------------------------------------------------------------
def _svgp(AGP, kernel=None, D=3, m=5, **kw):
    Z = np.random.default_rng(0).standard_normal((m, D))
    return AGP.SVGP(kernel or AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), Z, optimiser=False, **kw)


def test_python_refusals_and_argument_checks():
    """everything here is raised before the device is touched (there is none)"""
    import agp_amd as AGP

    X, box = np.zeros((4, 3)), (-1.0, 1.0)
    for model, match in ((_svgp(AGP, T=np.float32), "Float32"), (_svgp(AGP, AGP.ExponentialKernel()), "ExponentialKernel"),
                         (object(), "not a model")):
        with pytest.raises(NotImplementedError, match=match):
            AGP.acquisition(model, AGP.UCB(), X, pending=X[:2])
        with pytest.raises(NotImplementedError, match=match):
            AGP.maximize_acquisition_batch(model, AGP.UCB(), 2, X, box)
    model = _svgp(AGP)
    mb = lambda q=2, **kw: AGP.maximize_acquisition_batch(model, kw.pop("acq", AGP.UCB()), q, kw.pop("X0", X), kw.pop("bounds", box), **kw)
    for kw, match in ((dict(q=0), "q must be"), (dict(q=-1), "q must be"), (dict(q=2.0), "q must be"), (dict(q=True), "q must be"),
                      (dict(q=65), "exceed 64"), (dict(q=60, pending=np.zeros((5, 3))), "exceed 64"),
                      (dict(pending=np.zeros((2, 2))), r"pending must be"), (dict(pending=np.zeros(3)), r"pending must be"),
                      (dict(pending_noise=-0.1), "pending_noise"), (dict(pending_noise=float("nan")), "pending_noise"),
                      (dict(pending_noise=float("inf")), "pending_noise"), (dict(bounds=(1.0, -1.0)), "lo <= hi"), (dict(steps=-1), "steps"),
                      (dict(lr=0.0), "step sizes"), (dict(X0=np.zeros((4, 2))), "X0 must be"), (dict(X0=np.zeros((0, 3))), "starts"),
                      (dict(latent=3), "latent"), (dict(acq=AGP.EI()), "best=None")):
        with pytest.raises(ValueError, match=match):
            mb(**kw)
    with pytest.raises(TypeError, match="UCB"):
        mb(acq="ucb")
    for kw, match in ((dict(pending=np.zeros((2, 4))), "pending must be"), (dict(pending=np.zeros((64, 3))), "exceed 64"),
                      (dict(pending=X[:2], pending_noise=-1.0), "pending_noise")):
        with pytest.raises(ValueError, match=match):
            AGP.acquisition(model, AGP.UCB(), X, **kw)


def test_symbols_are_in_the_header_the_binding_and_the_shim():
    import agp_amd as AGP
    from agp_amd import capi

    text = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("agp_svgp_acquisition_pending", 13), ("agp_svgp_acq_maximize_batch", 16)):
        m = re.search(r"agp_status\s+" + name + r"\s*\(([^;]*)\);", h)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(capi.SYMBOLS[name][1]) == nargs
        assert name in open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    assert re.search(r"#define\s+AGP_ACQ_MAX_PENDING\s+64\b", h) and capi.ACQ_MAX_PENDING == 64
    assert callable(AGP.maximize_acquisition_batch)
    for phrase in ("C_ij   = cov(p_i, p_j) + (jitter + tau2) [i == j]", "var_P(x) = var(x) - c(x)' C^-1 c(x)",
                   "A'' = [[A' + w w'/c, -w/c], [-w'/c, 1/c]]", "c  = (v + jitter + tau2) - k'' w"):
        assert phrase in text, phrase
    assert "batch (q-) acquisition" not in text
