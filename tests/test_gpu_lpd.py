"""GPU: the log predictive density -- agp_log_predictive point by point against the 40-digit restatement (tests/golden/lpd/lpd_mp.npz,
tests/_lpd_ref.py), and the streamed agp_svgp_lpd_stream against the restatement fed with the oracle's predict_f(cov=True) (relative
1e-8, the project's parity bound) and with the device's own predict_f moments (1e-12 max(1, |ref|)).  Cases: tests/_lpd_cases.py.

fp32 (test_fp32, Logistic, n = 8229): e32, the error of the handle's own fp32 predict_f moments pushed through the float64
restatement, against the fp64 oracle, and the streamed fp32 value's error are printed; the latter must lie within 4 e32."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _lpd_cases as S
import _lpd_ref as Rf
from _pitched import Pitched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID, NEG_KTILDE, LABELS = 5, 1, 3, 6
SENT = -12345.5  # what sum_host holds before a call that must leave it untouched


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    return dict(torch=torch, AGP=AGP, capi=capi, R=R, L=capi.lib())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


GH = Rf.gh_rule(100)


def _stream(L, model, Xd, yd, n, vec=None, xptr=None, ldx=None, rule=GH):
    """(status, sum) of agp_svgp_lpd_stream on the first n points"""
    out = C.c_double(SENT)
    st = L.agp_svgp_lpd_stream(model._h, C.c_void_p(Xd.data_ptr() if xptr is None else xptr), Xd.stride(0) if ldx is None else ldx,
                               C.c_void_p(yd.data_ptr()), n, _dp(rule[0]), _dp(rule[1]), len(rule[0]), C.byref(out),
                               C.c_void_p(vec.data_ptr()) if vec is not None else None)
    return st, out.value


@functools.lru_cache(maxsize=None)
def _trained(name):
    """(model with a live handle, device test points, device treated labels) of a case, built once"""
    import agp_amd as AGP
    import torch

    o = S.trained_oracle(name)
    model = S.make_model(AGP, name)
    Xd = model._upload(o["Xt"])
    yd = torch.as_tensor(o["yt"], device="cuda").contiguous()
    model._ensure_handle(max(model._max_batch, 1))
    return model, Xd, yd


# ---- (c) the point-wise kernel on given moments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Rf.GRID_LIKS))
def test_log_predictive_point_by_point(env, name):
    """1000 points per likelihood (var from 1e-12 to 1e2, |mu| <= 30, the rows mu = -+800 y and |d| = 50), n_nodes in {1, 3, 20, 100,
    257}: fp64 against the mpmath restatement within 1e-12 max(1, |ref|)"""
    AGP = env["AGP"]
    g = np.load(os.path.join(ROOT, "tests", "golden", Rf.GOLDEN))
    y, mu, var = Rf.grid(name)
    lt = Rf.GRID_LIKS[name]
    lik = {"gaussian": lambda: AGP.GaussianLikelihood(lt[1]), "laplace": lambda: AGP.LaplaceLikelihood(lt[1]),
           "logistic": AGP.LogisticLikelihood, "bayesiansvm": AGP.BayesianSVM, "studentt": lambda: AGP.StudentTLikelihood(lt[1], lt[2]),
           "poisson": lambda: AGP.PoissonLikelihood(lt[1]), "negbinomial": lambda: AGP.NegBinomialLikelihood(lt[1]),
           "logisticsoftmax": lambda: AGP.LogisticSoftMaxLikelihood(lt[1]), "softmax": lambda: AGP.SoftMaxLikelihood(lt[1])}[name]()
    for n in (Rf.GRID_NODES if name in Rf.QUAD else (None,)):
        x, w = Rf.gh_rule(n) if n else (None, None)
        ref = g[f"{name}/lpd{n}" if n else f"{name}/lpd"]
        got = AGP.log_predictive_moments(lik, y, mu, var, x, w)
        assert got.shape == ref.shape and np.all(np.isfinite(got))
        err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"{name} n_nodes={n}: worst |device - mpmath| / max(1, |ref|) = {err:.2e}")
        assert err <= 1e-12
    if name == "logistic":
        assert np.all(np.abs(got[2:4] + 800.0) < 1.0)
    # fp32 moments: the same kernel, double accumulation (the inputs rounded to float: compared with the restatement on those)
    m32, v32 = mu.astype(np.float32), var.astype(np.float32)
    y32 = y if name in Rf.MULTI else y.astype(np.float32)
    x, w = Rf.gh_rule(20) if name in Rf.QUAD else (None, None)
    got32 = AGP.log_predictive_moments(lik, y32, m32, v32, x, w, dtype=np.float32)
    want = Rf.lpd_np(lt, y32.astype(np.float64) if name not in Rf.MULTI else y, m32.astype(np.float64), v32.astype(np.float64), x, w)
    assert got32.dtype == np.float32
    assert np.all(np.abs(got32 - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want)))  # one rounding of the result to float


# ---- (d) the streamed call ----------------------------------------------------------------------------------------------------------------
def _check_stream(env, model, Xd, yd, o, n, lik_tuple=None):
    """sum and vector of the first n points against the oracle-fed and the device-fed restatement"""
    torch, AGP, L = env["torch"], env["AGP"], env["L"]
    vec = torch.full((n,), float("nan"), dtype=model.tdtype, device="cuda")
    st, total = _stream(L, model, Xd, yd, n, vec)
    assert st == 0, L.agp_last_error(model._ctx)
    v = vec.cpu().numpy().astype(np.float64)
    want = o["lpd"][:n]
    e_sum = abs(total - want.sum()) / abs(want.sum())
    e_vec = float(np.max(np.abs(v - want) / np.maximum(1.0, np.abs(want))))
    mu, var = AGP.predict_f(model, o["Xt"][:n], cov=True)
    own = S.restated(lik_tuple or o["lik"], o["yt"][:n], np.asarray(mu), np.asarray(var))
    d_sum = abs(total - own.sum()) / max(1.0, abs(own.sum()))
    d_vec = float(np.max(np.abs(v - own) / np.maximum(1.0, np.abs(own))))
    p_sum = abs(total - v.sum()) / np.sum(np.abs(v))
    print(f"n={n}: vs oracle sum {e_sum:.2e} vector {e_vec:.2e}; vs own moments sum {d_sum:.2e} vector {d_vec:.2e}; "
          f"pointwise total {p_sum:.2e}")
    assert e_sum <= 1e-8 and e_vec <= 1e-8
    assert d_sum <= 1e-12 and d_vec <= 1e-12
    assert p_sum <= 1e-12
    # without the vector: the same bits
    assert _stream(L, model, Xd, yd, n) == (0, total)
    return total, v


STREAM = [("logistic", n) for n in S.NS] + [(c, S.CASES[c][5]) for c in S.CASES if c != "logistic"]


@pytest.mark.parametrize("name,n", STREAM)
def test_stream_parity_fp64(env, name, n):
    o = S.trained_oracle(name)
    model, Xd, yd = _trained(name)
    lt = o["lik"]
    if name == "poisson":  # the handle's CURRENT lambda (within the parity bound of the oracle's)
        lam = model.likelihood.lam
        assert abs(lam - lt[1]) <= 1e-8 * lt[1]
        lt = ("poisson", lam)
    _check_stream(env, model, Xd, yd, o, n, lt)
    assert model._max_batch == S.B


def test_every_likelihood_at_the_group_edges(env):
    """n in {1, 15, 16, 17, 4097}: below, on and above the 16-point workgroup of the quadrature kinds, and the second chunk"""
    for name in ("gaussian", "laplace", "bayesiansvm", "studentt", "poisson", "negbinomial", "logisticsoftmax"):
        o = S.trained_oracle(name)
        model, Xd, yd = _trained(name)
        lt = ("poisson", model.likelihood.lam) if name == "poisson" else o["lik"]
        for n in (1, 15, 16, 17, 4097):
            _check_stream(env, model, Xd, yd, o, n, lt)


def test_determinism_and_layout(env):
    torch, L = env["torch"], env["L"]
    o = S.trained_oracle("logistic")
    model, Xd, yd = _trained("logistic")
    n = S.NMAX
    va, vb = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
    a = _stream(L, model, Xd, yd, n, va)
    b = _stream(L, model, Xd, yd, n, vb)
    assert a[0] == 0 and a == b and torch.equal(va, vb)  # two calls: the same bits, sum and vector
    for ld, off in ((S.D + 1, 1), (64 + 64, 0)):
        px = Pitched("f64", data=o["Xt"], ld=ld, off=off, device="cuda")  # every element outside the window is a NaN
        vb.fill_(0.0)
        assert _stream(L, model, Xd, yd, n, vb, xptr=px.ptr, ldx=ld) == a and torch.equal(va, vb)
        px.check("x")
    # another rule, then the first again (the device copy of the rule follows the caller's)
    c = _stream(L, model, Xd, yd, n, rule=Rf.gh_rule(20))
    assert c[0] == 0 and c != a and abs(c[1] - a[1]) < 1e-3 * abs(a[1])
    assert _stream(L, model, Xd, yd, n) == a


def _vgp_like(env, kind):
    """(model, restatement's likelihood, treated test labels, oracle moments at the test points, test points)"""
    AGP, R = env["AGP"], env["R"]
    rng = np.random.default_rng(31)
    N, nt = 130, 300
    X = rng.standard_normal((N, S.D))
    Xt = rng.standard_normal((nt, S.D))
    f, ft = S._f(X), S._f(Xt)
    if kind == "vgp":
        from _vgp_ref import VGPRef

        y = (f + 0.3 * rng.standard_normal(N) > f.mean()).astype(np.int64)
        yt = np.sign((ft + 0.3 * rng.standard_normal(nt) > f.mean()) - 0.5)
        model = AGP.VGP(X, y, S.KVAR * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(S.KSCALE)), AGP.LogisticLikelihood(),
                        AGP.AnalyticVI(), optimiser=False)
        AGP.train_(model, 4)
        ref = VGPRef(R.Kernel("sqexponential", S.KSCALE, S.KVAR), R.LogisticLikelihood(), X)
        ytr = R.treat_labels(y, R.LogisticLikelihood())
        for _ in range(4):
            ref.step(ytr)
        mus, vars_, _ = ref.predict_f(Xt)
        return model, ("logistic",), yt, mus[0], vars_[0], Xt
    if kind == "gp":
        from _gp_ref import GPRef

        y = f + 0.2 * rng.standard_normal(N)
        yt = ft + 0.2 * rng.standard_normal(nt)
        model = AGP.GP(X, y, S.KVAR * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(S.KSCALE)), noise=0.05, opt_noise=True,
                       optimiser=False)
        AGP.train_(model, 5)
        ref = GPRef(R.Kernel("sqexponential", S.KSCALE, S.KVAR), X, y, noise=0.05, opt_noise=True)
        ref.train(5)
        mu, var, _ = ref.predict_f(Xt)
        return model, ("gaussian", float(ref.sigma2)), yt, mu, var, Xt
    import _nvi_cases as CS

    name = "studentt-svi-nat-descent"
    case = CS.SPARSE_CASES[name]
    Xs, ys, Z, idx = CS.sparse_data(case)
    inf = AGP.QuadratureSVI(CS.SPARSE["B"], nGaussHermite=100, optimiser=AGP.Descent(0.1), natural=True)
    model = AGP.SVGP(1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0)), AGP.StudentTLikelihood(3.0, 1.0), inf, Z, optimiser=False)
    AGP.train_(model, Xs, ys, CS.SPARSE["steps"], idx_stream=idx)
    ref = CS.sparse_trajectory(name)["ref"]
    Xt = rng.standard_normal((nt, CS.SPARSE["D"]))
    yt = S._f(Xt) + 0.2 * rng.standard_t(3, nt)
    mu, var = ref.predict_f(Xt)
    return model, ("studentt", 3.0, 1.0), yt, mu, var, Xt


@pytest.mark.parametrize("kind", ["vgp", "gp", "quadrature-svgp"])
def test_other_model_classes(env, kind):
    """one routine serves every class whose predict_f works: a VGP (N = 130), a GP (with its optimised noise), a QuadratureVI SVGP"""
    torch, AGP, L = env["torch"], env["AGP"], env["L"]
    model, lt, yt, mu, var, Xt = _vgp_like(env, kind)
    if kind == "gp":  # the handle's CURRENT noise (the opt_noise state)
        assert abs(model.likelihood.sigma2 - lt[1]) <= 1e-8 * lt[1] and lt[1] != 0.05
    want = S.restated(lt, yt, np.asarray(mu), np.asarray(var))
    total, vec = AGP.log_predictive_density(model, Xt, yt if kind != "vgp" else (yt > 0).astype(np.int64), pointwise=True)
    e_sum = abs(total - want.sum()) / abs(want.sum())
    e_vec = float(np.max(np.abs(vec - want) / np.maximum(1.0, np.abs(want))))
    dm, dv = AGP.predict_f(model, Xt, cov=True)
    if kind == "gp":
        lt = ("gaussian", model.likelihood.sigma2)
    own = S.restated(lt, yt, np.asarray(dm), np.asarray(dv))
    d_vec = float(np.max(np.abs(vec - own) / np.maximum(1.0, np.abs(own))))
    print(f"{kind}: vs restated reference sum {e_sum:.2e} vector {e_vec:.2e}; vs own moments vector {d_vec:.2e}")
    assert e_sum <= 1e-8 and e_vec <= 1e-8
    assert d_vec <= 1e-12 and abs(total - own.sum()) <= 1e-12 * max(1.0, abs(own.sum()))
    assert AGP.log_predictive_density(model, Xt, yt if kind != "vgp" else (yt > 0).astype(np.int64)) == total


# ---- (e) fp32 ---------------------------------------------------------------------------------------------------------------------------
def test_fp32(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    o = S.trained_oracle("logistic", jitter=1e-3)  # the oracle with the reference's Float32 jitter
    model = S.make_model(AGP, "logistic", T=np.float32)
    n = S.NMAX
    want = o["lpd"].sum()
    mu, var = AGP.predict_f(model, o["Xt"], cov=True)
    e32 = abs(S.restated(o["lik"], o["yt"], np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)).sum() - want) / abs(want)
    Xd = model._upload(o["Xt"])
    yd = torch.as_tensor(o["yt"], dtype=torch.float32, device="cuda")
    vec = torch.empty(n, dtype=torch.float32, device="cuda")
    st, total = _stream(L, model, Xd, yd, n, vec)
    assert st == 0, L.agp_last_error(model._ctx)
    es = abs(total - want) / abs(want)
    print(f"fp32: own-moments error e32 = {e32:.3e}, streamed error = {es:.3e}, ratio {es / e32:.2f}")
    assert es <= 4 * e32
    assert abs(float(vec.double().sum()) - total) <= 1e-6 * abs(total)


# ---- (f) side effects and failure -------------------------------------------------------------------------------------------------------
def _snapshot(env, model):
    capi, L = env["capi"], env["L"]
    terms = (C.c_double * 3)()
    model._chk(L.agp_svgp_elbo_terms(model._h, terms))
    snap = [np.asarray(tuple(terms))]
    for l in range(model.n_latent):
        snap += list(model.get_state(l))
        snap += [model.get_matrix(w, l) for w in (capi.VEC_THETA, capi.VEC_C, capi.VEC_MEAN_F)]
    return snap


@pytest.mark.parametrize("name", ["logistic", "logisticsoftmax"])
def test_no_side_effects(env, name):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    o = S.trained_oracle(name)
    model = S.make_model(AGP, name)
    Xd = model._upload(o["Xt"])
    yd = torch.as_tensor(o["yt"], device="cuda")
    e0 = AGP.objective(model)  # agp_svgp_elbo(fresh_local = 0) on the last batch; what agp_svgp_elbo_terms then refers to
    before = _snapshot(env, model)
    st, v = _stream(L, model, Xd, yd, S.NMAX)
    assert st == 0
    assert L.agp_svgp_check_status(model._h) == 0
    after = _snapshot(env, model)
    e1 = AGP.objective(model)
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                     b.view(np.uint64) if b.dtype == np.float64 else b)
    assert e0 == e1


def test_workspace_does_not_grow_with_n(env):
    """free device memory after a call at n = 8229 and after one at n = 20481: only the partial sums grow, at most one byte per
    point, rounded up to the allocator's granularity (2 MiB)"""
    torch, L = env["torch"], env["L"]
    model, Xd, yd = _trained("logistic")
    n2 = 5 * 4096 + 1
    rep = -(-n2 // len(Xd))
    X2 = torch.cat([Xd] * rep)[:n2].contiguous()
    y2 = torch.cat([yd] * rep)[:n2].contiguous()
    assert _stream(L, model, Xd, yd, S.NMAX)[0] == 0
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    st, v = _stream(L, model, X2, y2, n2)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    assert st == 0 and np.isfinite(v)
    gran = 2 << 20
    bound = -(-n2 // gran) * gran
    print(f"free memory {free1} -> {free2}: {free1 - free2} bytes, bound {bound}")
    assert free1 - free2 <= bound


def test_failures_name_the_first_position(env):
    torch, L, AGP = env["torch"], env["L"], env["AGP"]
    model, Xd, yd = _trained("logistic")
    n = S.NMAX
    st, good = _stream(L, model, Xd, yd, n)
    assert st == 0
    bad = Xd.clone()
    for where in (7000, 4353):  # 4353: second chunk, off the 16- and 256-grids
        bad[where, 1] = float("nan")
    st, v = _stream(L, model, bad, yd, n)
    msg = L.agp_last_error(model._ctx).decode()
    assert st == NEG_KTILDE and v == SENT, (st, msg)
    assert "point 4353 " in msg and "agp_svgp_lpd_stream" in msg, msg
    ybad = yd.clone()
    ybad[4100] = 0.0
    ybad[6000] = 0.0
    st, v = _stream(L, model, Xd, ybad, n)
    msg = L.agp_last_error(model._ctx).decode()
    assert st == LABELS and v == SENT and "point 4100 " in msg, (st, msg)
    assert L.agp_svgp_check_status(model._h) == 0  # nothing latched
    assert _stream(L, model, Xd, yd, n) == (0, good)
    for name, where, val in (("poisson", 4200, 2.5), ("logisticsoftmax", 17, 3)):
        m2, X2, y2 = _trained(name)
        yb = y2.clone()
        yb[where] = val
        st, v = _stream(L, m2, X2, yb, n)
        msg = L.agp_last_error(m2._ctx).decode()
        assert st == LABELS and v == SENT and f"point {where} " in msg, (name, st, msg)
    # arguments
    assert _stream(L, model, Xd, yd, 0) == (0, 0.0)  # n = 0 succeeds with sum 0
    assert _stream(L, model, Xd, yd, -1) == (INVALID, SENT)
    assert _stream(L, model, Xd, yd, n, ldx=S.D - 1) == (INVALID, SENT)
    assert _stream(L, model, Xd, yd, n, rule=(GH[0][:0], GH[1][:0])) == (INVALID, SENT)
    x5000 = np.zeros(5000)
    assert _stream(L, model, Xd, yd, n, rule=(x5000, x5000 + 1.0)) == (INVALID, SENT)
    assert L.agp_svgp_lpd_stream(model._h, None, S.D, C.c_void_p(yd.data_ptr()), n, _dp(GH[0]), _dp(GH[1]), 100, None, None) == INVALID
    assert _stream(L, model, Xd, yd, n) == (0, good)


def test_refused_handles_through_the_abi(env):
    torch, L, AGP = env["torch"], env["L"], env["AGP"]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 2))
    yb = np.where(X[:, 0] > 0, 1, -1)
    yc = 1 + (np.arange(40) % 3)
    Z = X[:6].copy()
    k = AGP.SqExponentialKernel()
    svi = lambda: AGP.AnalyticSVI(20)  # noqa: E731
    handles = []

    def sparse(name, lik, yy, **kw):
        m = AGP.SVGP(k, lik, svi(), Z, optimiser=False, **kw)
        m._ensure_handle(20)
        handles.append((name, m, yy))
        return m

    sparse("Heteroscedastic", AGP.HeteroscedasticLikelihood(1.0), X[:, 1])
    sparse("latent-sharded", AGP.LogisticSoftMaxLikelihood(3), yc, latent_slice=(0, 2))
    sh = sparse("batch-sharded", AGP.LogisticLikelihood(), yb)
    sh._chk(L.agp_svgp_set_batch_shard(sh._h, 0, 2))
    mo = AGP.MOSVGP(k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], svi(), [Z, Z], optimiser=False)
    mo._ensure_handle(20)
    handles.append(("AGP_LIK_MULTIOUTPUT", mo, yb))
    mc = AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    handles.append(("AGP_FLAG_SAMPLED", mc, yb))
    for name, model, yy in handles:
        Xd = torch.as_tensor(X, dtype=model.tdtype, device="cuda")
        yd = torch.as_tensor(np.asarray(yy, dtype=np.float64), dtype=model.tdtype, device="cuda")
        st, v = _stream(L, model, Xd, yd, len(X))
        msg = L.agp_last_error(model._ctx).decode()
        assert st == UNSUPPORTED, (name, st, msg)
        assert "agp_svgp_lpd_stream" in msg and name in msg, (name, msg)
        assert v == SENT, name
    # an online handle and an AGP_FLAG_STALE_K handle are served
    on = AGP.OnlineSVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), AGP.OIPS(0.7), optimiser=False)
    for b in (0, 20):
        AGP.train_online(on, X[b:b + 20], yb[b:b + 20], iterations=2)
    stale = AGP.SVGP(k, AGP.LogisticLikelihood(), svi(), Z, optimiser=False, reference_compat_stale_K=True)
    AGP.train_(stale, X, yb, 3)
    for model in (on._cur, stale):
        total, vec = AGP.log_predictive_density(model, X, yb, pointwise=True)
        mu, var = AGP.predict_f(model, X, cov=True)
        own = S.restated(("logistic",), yb.astype(np.float64), np.asarray(mu), np.asarray(var))
        assert float(np.max(np.abs(vec - own))) <= 1e-12 and abs(total - own.sum()) <= 1e-12 * abs(own.sum())
