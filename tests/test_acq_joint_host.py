"""CPU tests of the joint Monte-Carlo batch acquisition (include/agp_hip.h, "ACQUISITION FUNCTIONS", paragraph "Joint batches"): the
restatement's tangent gradient against central differences of its own alpha, the kink condition and the yardstick's own rounding on
every input the GPU suite compares (on the oracle's objects: float64 against long double, 100 times below PARITY for values and
gradients, COND_CAP over a trajectory, so that neither a kink nor rounding in the yardstick can decide a GPU test), the q = 1
identities, the symbols, and the host mirror's argument checks.
"""
import os
import re

import numpy as np
import pytest

import _acq_joint_ref as J
import _acq_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK = A.PARITY / 100  # float64 against long double of the restatement
LD = np.longdouble


# ---- 1. the gradient is the derivative of the restatement's own alpha ----------------------------------------------------------------------
@pytest.mark.parametrize("name,q,n", [("m65-logistic-m32-ard", 3, 0), ("gp", 2, 2), ("d5", 1, 3), ("vgp", 4, 1)])
@pytest.mark.parametrize("kind,minimize", J.DIRECTIONS)
def test_gradient_against_central_differences(name, q, n, kind, minimize):
    """in long double with h = 1e-5 of the spread: the truncation is h^2 |alpha'''| / 6, about 1e-10 of the gradient, the rounding
    1e-19 / h.  A difference quotient must not cross a kink, so the sets are those of a drawn pool whose margin exceeds 1e-3 -- a
    hundred times what a step of h can move a sample's value; the pool is this test's own, not an input of the GPU suite."""
    parts = A.oracle_parts(name)
    X, P = J.sets(name, q, n, 24, 3)
    eps = J.table(9, q + n, 3)
    acq = J.case_acq(kind, minimize, X, P, parts)
    al, g, margin = J.alpha_grad(acq, X, parts, eps, P, dtype=LD)
    keep = np.flatnonzero(margin > 1e-3)[:3]
    assert len(keep) == 3, margin
    X, g = X[keep], g[keep]
    h = LD(1e-5) * LD(J._box(name)[1])
    fd = np.zeros_like(g)
    for j in range(q):
        for d in range(X.shape[2]):
            Xp, Xm = X.astype(LD), X.astype(LD)
            Xp[:, j, d] += h
            Xm[:, j, d] -= h
            ap = _alpha_ld(acq, Xp, parts, eps, P)
            am = _alpha_ld(acq, Xm, parts, eps, P)
            fd[:, j, d] = (ap - am) / (2 * h)
    err = A.relerr(fd, g)
    print(f"{name} q={q} n={n} {kind} minimize={minimize}: tangent gradient against central differences {err:.2e}")
    assert np.max(np.abs(g)) > 0 and err <= 1e-7


def _alpha_ld(acq, X, parts, eps, P):
    """alpha at long-double points (alpha_grad takes float64 inputs: the moments are formed here)"""
    Z, sc, v, kind, a, Ap = J._cast(parts, LD)
    Xa = np.concatenate([X, np.broadcast_to(np.asarray(P, dtype=LD)[None], (len(X),) + P.shape)], axis=1) if len(P) else X
    n, qp, D = Xa.shape
    K = (v * J.G.phi(kind, J.G.sqdist(Xa.reshape(n * qp, D), Z, sc))).reshape(n, qp, -1)
    _, qq = J._pairs(Xa, sc)
    C = J.from_lower(v * J.G.phi(kind, qq) - K @ Ap @ np.swapaxes(K, 1, 2) + LD(J.JITTER) * np.eye(qp, dtype=LD))
    term = J.samples(acq, K @ a, J.chol(C), eps, LD)[0]
    return np.sum(term, axis=1) / LD(term.shape[1])


def test_the_moments_are_those_of_the_predictor():
    """mu and the diagonal of C are the mean and variance of _acq_ref.moments; C is symmetric and positive definite"""
    name = "m65-logistic-m32-ard"
    parts = A.oracle_parts(name)
    X, P = J.sets(name, 3, 2, 6, 0)
    mu, C, _ = J.moments(X, parts, P)
    wm, wv = A.moments(J.members(X, P).reshape(-1, X.shape[2]), *parts)
    assert A.relerr(mu.ravel(), wm) <= 1e-14 and A.relerr(np.einsum("njj->nj", C).ravel(), wv) <= 1e-12
    assert np.array_equal(C, np.swapaxes(C, 1, 2)) and np.all(np.linalg.eigvalsh(C) > 0)
    L = J.chol(C)
    assert A.relerr(L @ np.swapaxes(L, 1, 2), C) <= 1e-14 and A.relerr(L, np.linalg.cholesky(C)) <= 1e-12


# ---- 2. the kink condition and the rounding of the yardstick, on every input of the GPU suite ---------------------------------------------------
@pytest.mark.parametrize("case", J.VALUES, ids=J.value_id)
def test_kinks_and_rounding_of_the_value_inputs(case):
    name, q, n, S, nsets, seed = case
    parts = A.oracle_parts(name)
    X, P = J.sets(name, q, n, nsets, seed)
    if nsets > 600:  # the chunk case in long double: the first and the last sets (the GPU suite asserts the condition on all of them)
        X = np.concatenate([X[:100], X[-100:]])
    eps = J.table(S, q + n, seed)
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, X, P, parts)
        a64, g64, m64 = J.alpha_grad(acq, X, parts, eps, P)
        ald, gld, mld = J.alpha_grad(acq, X, parts, eps, P, dtype=LD)
        ea, eg = A.relerr(a64, ald), A.relerr(g64, gld)
        print(f"{J.value_id(case)} {kind} minimize={minimize}: margin {float(np.min(m64)):.2e}  alpha {ea:.2e}  grad {eg:.2e}")
        assert float(np.min(m64)) > J.KINK and float(np.min(mld)) > J.KINK  # no case may be left out: all of them hold
        assert ea <= YARDSTICK and eg <= YARDSTICK


def test_the_value_inputs_have_their_edges():
    qs, Ss, ns = {c[1] for c in J.VALUES}, {c[3] for c in J.VALUES}, {(c[1], c[2]) for c in J.VALUES}
    assert qs == {1, 2, 3, 16} and Ss == {1, 63, 64, 65, 257}
    assert all(any(k == q and m == v for k, m in ns) for q in (1, 2, 3) for v in (16 - q,)) and {n for _, n in ns} >= {0, 1}
    assert {c[0] for c in J.VALUES} == {"m1-r1", "d1-m63-r63", "d64-m64-r64", "m65-logistic-m32-ard", "gp", "vgp", "online"}
    assert any(c[1] == 3 and c[4] == 1366 for c in J.VALUES) and 4096 // 3 == 1365  # a ragged tuple at the chunk boundary


@pytest.mark.parametrize("name,T", J.ASCENTS)
def test_kinks_and_conditioning_of_the_ascents(name, T):
    parts = A.oracle_parts(name)
    X0, P, lo, hi, lr = J.ascent_inputs(name)
    eps = J.table(J.ASCENT_S, J.ASCENT_Q + 1)
    box = float(np.max(hi - lo))
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, np.minimum(np.maximum(X0, lo), hi), P, parts)
        for pend in (P, None):
            e = eps if pend is not None else eps[:, :J.ASCENT_Q]
            x64, a64, m64 = J.ascent(acq, X0, parts, e, lo, hi, lr, T, pend)
            xld, ald, mld = J.ascent(acq, X0, parts, e, lo, hi, lr, T, pend, dtype=LD)
            cx, ca, gap = float(np.max(np.abs(x64 - xld)) / box), A.relerr(a64, ald), A.top_gap(a64)
            print(f"{name} T={T} {kind} minimize={minimize} pending={pend is not None}: margin {m64:.2e}  x {cx:.1e}  alpha {ca:.1e}  gap {gap:.1e}")
            assert m64 > J.KINK and mld > J.KINK
            assert cx <= A.COND_CAP and ca <= A.COND_CAP
            assert gap > A.GAP
            assert np.all(x64 >= lo) and np.all(x64 <= hi)


@pytest.mark.parametrize("name", ["m65-logistic-m32-ard", "d1-m63-r63"])
def test_conditioning_of_the_degenerate_sets(name):
    """two identical members leave C with an eigenvalue of about the jitter: the factor's tangent then carries 1 / jitter, and the
    gradient's own rounding is what this test states for the GPU suite (test_gpu_acq_joint.test_degenerate_sets): values within
    PARITY / 100, gradients within DEGENERATE_GRAD / 100"""
    parts = A.oracle_parts(name)
    assert A.spec(name)["kind"] in ("matern32", "matern52")
    X, P = J.degenerate(name)
    eps = J.table(64, 4, 5)
    for kind, minimize in J.DIRECTIONS:
        acq = J.case_acq(kind, minimize, X, P, parts)
        a64, g64, m64 = J.alpha_grad(acq, X, parts, eps, P)
        ald, gld, _ = J.alpha_grad(acq, X, parts, eps, P, dtype=LD)
        ea, eg = A.relerr(a64, ald), A.relerr(g64, gld)
        cond = float(np.max(np.linalg.cond(J.moments(X, parts, P)[1])))
        print(f"{name} {kind} minimize={minimize}: cond(C) {cond:.1e}  margin {float(np.min(m64)):.2e}  alpha {ea:.2e}  grad {eg:.2e}")
        assert np.all(np.isfinite(a64)) and np.all(np.isfinite(g64)) and float(np.min(m64)) > J.KINK
        assert ea <= YARDSTICK and eg <= DEGENERATE_GRAD / 100


# the gradient bound of the degenerate sets: eps cond(C)^(3/2) with cond(C) <= q' (v + jitter) / jitter ~ 4e4 at q' = 4 -- the tangent
# d L = L Phi(L^-1 dC L^-T) applies L^-1 twice to a dC whose own cancellation is relative to |C| -- is 2.2e-16 * 8e6 = 2e-9 for the
# yardstick in float64; the device sums in another order, so the GPU suite compares within 100 times that.
DEGENERATE_GRAD = 2e-7


# ---- 3. q' = 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ei", "ucb"])
def test_one_member_is_the_sample_average_of_the_point_function(kind):
    """q = 1, n = 0: alpha = mean_s (imp + sigma eps_s)^+ (q-EI) and s mu + beta sqrt(pi/2) sigma mean|eps| (q-UCB); with the 4096
    draws of the seed it lies within five Monte-Carlo standard errors of the analytic EI / UCB, the standard error being that of
    the same table (J.one_member_inputs keeps |z| <= 2, where a table of 4096 draws estimates its own standard error)"""
    name = "m65-logistic-m32-ard"
    parts = A.oracle_parts(name)
    X, acq = J.one_member_inputs(name, kind, parts)
    eps = J.base_samples(4096, 1, 0)
    al, _, _ = J.alpha_grad(acq, X, parts, eps, grad=False)
    mu, var = A.moments(X[:, 0], *parts)
    terms = J.one_member_terms(acq, mu, var, eps)
    assert A.relerr(al, terms.mean(axis=1)) <= 1e-13
    se = terms.std(axis=1, ddof=1) / np.sqrt(4096)
    exact = A.point(acq, mu, var)[0]
    print(f"{kind}: {len(X)} points, largest |alpha - exact| / se = {float(np.max(np.abs(al - exact) / se)):.2f}")
    assert len(X) >= 20 and np.all(se > 0) and np.all(np.abs(al - exact) <= 5 * se)


# ---- 4. the host mirror and the symbols ---------------------------------------------------------------------------------------------------------
def _svgp(AGP, kernel=None, D=3, m=5, **kw):
    Z = np.random.default_rng(0).standard_normal((m, D))
    return AGP.SVGP(kernel or AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), Z, optimiser=False, **kw)


def test_python_refusals_and_argument_checks():
    """everything here is raised before the device is touched (there is none)"""
    import agp_amd as AGP

    X, box = np.zeros((4, 2, 3)), (-1.0, 1.0)
    for model, match in ((_svgp(AGP, T=np.float32), "Float32"), (_svgp(AGP, AGP.ExponentialKernel()), "ExponentialKernel"),
                         (object(), "not a model")):
        with pytest.raises(NotImplementedError, match=match):
            AGP.acquisition_joint(model, AGP.UCB(), X)
        with pytest.raises(NotImplementedError, match=match):
            AGP.maximize_acquisition_joint(model, AGP.UCB(), X, box)
    model = _svgp(AGP)
    for acq, match in ((AGP.PI(0.0), "PI"), (AGP.LogEI(0.0), "LogEI"), (AGP.LogPI(0.0), "LogPI")):
        with pytest.raises(NotImplementedError, match=match + " has no joint form"):
            AGP.acquisition_joint(model, acq, X)
        with pytest.raises(NotImplementedError, match=match + " has no joint form"):
            AGP.maximize_acquisition_joint(model, acq, X, box)
    ev = lambda **kw: AGP.acquisition_joint(model, kw.pop("acq", AGP.UCB()), kw.pop("Xq", X), **kw)
    mx = lambda **kw: AGP.maximize_acquisition_joint(model, kw.pop("acq", AGP.UCB()), kw.pop("X0", X), kw.pop("bounds", box), **kw)
    shared = ((dict(pending=np.zeros((15, 3))), "exceed 16"), (dict(pending=np.zeros((2, 2))), "pending must be"),
              (dict(pending=np.zeros(3)), "pending must be"), (dict(samples=0), r"\[1, 4096\]"), (dict(samples=4097), r"\[1, 4096\]"),
              (dict(samples=2.5), "samples must be"), (dict(seed=-1), "seed"), (dict(base_samples=np.zeros((8, 3))), "base_samples must be"),
              (dict(base_samples=np.zeros((4097, 2))), r"\[1, 4096\]"), (dict(base_samples=np.zeros(8)), "base_samples must be"),
              (dict(latent=3), "latent"), (dict(acq=AGP.EI()), "best=None"))
    for kw, match in shared:
        with pytest.raises(ValueError, match=match):
            ev(**dict(kw))
        with pytest.raises(ValueError, match=match):
            mx(**dict(kw))
    for kw, match in ((dict(Xq=np.zeros((4, 3))[:, None, :2]), "Xq must be"), (dict(Xq=np.zeros(3)), "Xq must be"),
                      (dict(Xq=np.zeros((2, 17, 3))), "exceed 16"), (dict(Xq=np.zeros((2, 0, 3))), "at least one point")):
        with pytest.raises(ValueError, match=match):
            ev(**kw)
    for kw, match in ((dict(X0=np.zeros((4, 3))), "X0 must be"), (dict(X0=np.zeros((4, 2, 2))), "X0 must be"),
                      (dict(X0=np.zeros((0, 2, 3))), "starts"), (dict(X0=np.zeros((2, 17, 3))), "exceed 16"),
                      (dict(bounds=(1.0, -1.0)), "lo <= hi"), (dict(steps=-1), "steps"), (dict(lr=0.0), "step sizes")):
        with pytest.raises(ValueError, match=match):
            mx(**kw)
    with pytest.raises(TypeError, match="EI"):
        ev(acq="ei")
    with pytest.raises(TypeError, match="grad is a bool"):
        ev(grad=1)


def test_symbols_are_in_the_header_the_binding_and_the_shim():
    import agp_amd as AGP
    from agp_amd import capi

    text = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    julia = open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
    for name, nargs in (("agp_svgp_acquisition_joint", 16), ("agp_svgp_acq_maximize_joint", 21)):
        m = re.search(r"agp_status\s+" + name + r"\s*\(([^;]*)\);", h)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(capi.SYMBOLS[name][1]) == nargs
        assert ":" + name in julia
        assert h.index("agp_svgp_acq_maximize_batch(") < h.index(name + "(")  # declared below the greedy batch
    assert re.search(r"#define\s+AGP_ACQ_JOINT_MAX_Q\s+16\b", h) and capi.ACQ_JOINT_MAX_Q == 16
    assert "an interface limit, not a tuned value" in text.split("AGP_ACQ_JOINT_MAX_Q 16")[1].split("\n")[0]
    assert callable(AGP.acquisition_joint) and callable(AGP.maximize_acquisition_joint)
    assert "Joint batches" in text
    for phrase in ("C_jl  = k(x_j, x_l) - k*(x_j)' A k*(x_l) + jitter [j == l]", "f_s   = mu + L eps_s",
                   "alpha = (1/S) sum_s max(0, max_j (s (f_sj - best) - xi))",
                   "alpha = (1/S) sum_s max_j (s mu_j + beta sqrt(pi/2) |(L eps_s)_j|)",
                   "Phi       = tril(L' L-bar) with the diagonal halved,   C-bar = sym(L^-T Phi L^-1)",
                   "V_j       = mu-bar_j a - 2 sum_l C-bar_jl W_l"):
        assert phrase in text, phrase
    assert "MC q-EI with a joint reparameterised sample, fantasies" not in text  # (no longer out of scope)
    ctypes_size = __import__("ctypes").sizeof(capi.AcqDesc)
    assert ctypes_size == 32  # agp_acq_desc keeps its 32 bytes: q, S and the base samples are separate arguments


def test_the_default_base_samples_are_reproducible_on_the_host():
    """the mirror's table is agp_mc_normals(seed, t=0, stream=3): tests/_mcvi_ref.py restates it"""
    import sys

    import agp_amd as AGP

    Q = sys.modules[AGP.acquisition_joint.__module__]
    assert Q.JOINT_STREAM == J.STREAM == 3
    E = J.base_samples(65, 4, 11)
    assert E.shape == (65, 4) and np.all(np.isfinite(E)) and abs(float(E.mean())) < 0.3 and 0.7 < float(E.std()) < 1.3
    assert np.array_equal(E, J.base_samples(65, 4, 11)) and not np.array_equal(E, J.base_samples(65, 4, 12))
