"""GPU: the streamed full-data ELBO (agp_svgp_elbo_stream) against the oracle's elbo_fresh and against the library's own one-batch
agp_svgp_elbo(fresh_local = 1) on a second handle created with max_batch = N.  fp64 bound: relative 1e-8 (the project's
device-versus-oracle bound); terms relative to max(1, |term|).  Cases, data and the oracle restatement: tests/_elbo_stream_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import _elbo_stream_cases as S
from _pitched import Pitched

pytestmark = pytest.mark.gpu

TOL = 1e-8
UNSUPPORTED, INVALID, NEG_KTILDE, BAD_BATCH = 5, 1, 3, 4
SENT = -12345.5  # what the outputs hold before a call that must leave them untouched


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    return dict(torch=torch, AGP=AGP, capi=capi, R=R, L=capi.lib())


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(model on a handle with max_batch = 150, twin for the one-batch evaluation, device x, device y) of a case, built once"""
    import agp_amd as AGP

    X, y, yt, Z, idx, ref = S.trained_oracle(name)
    model, twin = S.make_model(AGP, name), S.make_model(AGP, name)
    Xd = model._upload(X)
    yd = model._upload_y(model._treat(y))
    return model, twin, Xd, yd


def _stream(L, model, Xd, yd, n, rho=1.0, idx=None, xptr=None, ldx=None):
    out, terms = C.c_double(SENT), (C.c_double * 3)(SENT, SENT, SENT)
    st = L.agp_svgp_elbo_stream(model._h, C.c_void_p(Xd.data_ptr() if xptr is None else xptr), Xd.stride(0) if ldx is None else ldx,
                                C.c_void_p(yd.data_ptr()), C.c_void_p(idx.data_ptr()) if idx is not None else None, n, rho,
                                C.byref(out), terms)
    return st, out.value, tuple(terms)


def _one_batch(L, twin, Xd, yd, n, rho=1.0, idx=None):
    h = twin._ensure_handle(max(n, twin._max_batch))
    out, terms = C.c_double(), (C.c_double * 3)()
    twin._chk(L.agp_svgp_elbo(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()),
                              C.c_void_p(idx.data_ptr()) if idx is not None else None, n, rho, 1, C.byref(out)))
    twin._chk(L.agp_svgp_elbo_terms(h, terms))
    return out.value, tuple(terms)


def _errors(got_v, got_t, want_v, want_t):
    ev = abs(got_v - want_v) / abs(want_v)
    et = max(abs(g - w) / max(1.0, abs(w)) for g, w in zip(got_t, want_t))
    return ev, et


PARITY = [("logistic", n) for n in (1, 63, 4096, 4097, 8229)] + [(c, 4133) for c in (
    "gaussian", "studentt", "laplace", "bayesiansvm", "negbinomial", "logisticsoftmax", "logistic-ref", "laplace-ref",
    "logisticsoftmax-ref", "ard-matern52", "prior-mean")] + [("d130", 200)]


@pytest.mark.parametrize("name,n", PARITY)
def test_parity_fp64(env, name, n):
    L = env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle(name)
    model, twin, Xd, yd = _pair(name)
    assert model._max_batch == min(S.B, len(X))
    rho = 2.5
    st, v, t = _stream(L, model, Xd, yd, n, rho)
    assert st == 0, L.agp_last_error(model._ctx)
    assert model._max_batch == min(S.B, len(X))
    want_t = S.restated_terms(ref, X[:n], yt[:n])
    want_v = ref.elbo_fresh(X[:n], yt[:n], rho)
    ev, et = _errors(v, t, want_v, want_t)
    v1, t1 = _one_batch(L, twin, Xd, yd, n, rho)
    ev1, et1 = _errors(v, t, v1, t1)
    print(f"{name} n={n}: vs oracle value {ev:.2e} terms {et:.2e}; vs one-batch value {ev1:.2e} terms {et1:.2e}")
    assert abs(v - (rho * t[0] - t[1] - rho * t[2])) <= 1e-12 * abs(v)
    assert ev <= TOL and et <= TOL
    assert ev1 <= TOL and et1 <= TOL


def test_parity_with_idx(env):
    """idx: a random permutation of a 5000-point subset of the 8229 points"""
    torch, L = env["torch"], env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle("logistic")
    model, twin, Xd, yd = _pair("logistic")
    perm = np.random.default_rng(3).permutation(len(X))[:5000]
    pd = torch.as_tensor(perm, dtype=torch.int64, device="cuda")
    st, v, t = _stream(L, model, Xd, yd, 5000, 1.0, idx=pd)
    assert st == 0, L.agp_last_error(model._ctx)
    ev, et = _errors(v, t, ref.elbo_fresh(X[perm], yt[perm], 1.0), S.restated_terms(ref, X[perm], yt[perm]))
    twin._ensure_handle(len(X))
    v1, t1 = _one_batch(L, twin, Xd, yd, 5000, 1.0, idx=pd)
    ev1, et1 = _errors(v, t, v1, t1)
    print(f"idx: vs oracle value {ev:.2e} terms {et:.2e}; vs one-batch value {ev1:.2e} terms {et1:.2e}")
    assert max(ev, et, ev1, et1) <= TOL


def test_determinism_and_layout(env):
    torch, L = env["torch"], env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle("logistic")
    model, twin, Xd, yd = _pair("logistic")
    n = len(X)
    a = _stream(L, model, Xd, yd, n)
    b = _stream(L, model, Xd, yd, n)
    assert a[0] == 0 and a == b  # two calls: the same bits
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    assert _stream(L, model, Xd, yd, n, idx=ar) == a  # idx = arange(n) is idx = NULL
    for ld, off in ((S.D + 1, 1), (64 + 64, 0)):
        px = Pitched("f64", data=X, ld=ld, off=off, device="cuda")  # every element outside the window is a NaN
        assert _stream(L, model, Xd, yd, n, xptr=px.ptr, ldx=ld) == a
        assert _stream(L, model, Xd, yd, n, idx=ar, xptr=px.ptr, ldx=ld) == a
        px.check("x")


def _snapshot(env, model):
    AGP, capi, L = env["AGP"], env["capi"], env["L"]
    terms = (C.c_double * 3)()
    model._chk(L.agp_svgp_elbo_terms(model._h, terms))
    snap = [np.asarray(tuple(terms))]
    for l in range(model.n_latent):
        snap += list(model.get_state(l))
        snap += [model.get_matrix(w, l) for w in (capi.VEC_THETA, capi.VEC_C, capi.VEC_MEAN_F)]
    return snap


@pytest.mark.parametrize("name", ["logistic", "logisticsoftmax"])
def test_no_side_effects(env, name):
    AGP, L = env["AGP"], env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle(name)
    model = S.make_model(AGP, name)
    Xd = model._upload(X)
    yd = model._upload_y(model._treat(y))
    e0 = AGP.objective(model)  # agp_svgp_elbo(fresh_local = 0) on the last batch; what agp_svgp_elbo_terms then refers to
    before = _snapshot(env, model)
    st, v, t = _stream(L, model, Xd, yd, len(X))
    assert st == 0
    assert L.agp_svgp_check_status(model._h) == 0
    after = _snapshot(env, model)
    e1 = AGP.objective(model)
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                     b.view(np.uint64) if b.dtype == np.float64 else b)
    assert e0 == e1


def test_training_run_with_streamed_evaluations(env):
    """two 20-step SVI runs on one index stream, one with a streamed evaluation after every step: the posteriors agree to 1e-10
    relative (the bound of tests/test_gpu_round4.py for runs that differ only in where the pending step is completed)"""
    AGP = env["AGP"]
    likname, N = "logistic", 4133
    X, y, Z, _ = S.data(likname, N)
    rng = np.random.default_rng(11)
    idx = [np.sort(rng.choice(N, S.B, replace=False)) for _ in range(20)]
    runs, seen = [], []
    for evaluate in (False, True):
        model = AGP.SVGP(S.KVAR * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(S.KSCALE)), AGP.LogisticLikelihood(),
                         AGP.AnalyticSVI(S.B), Z, optimiser=False)
        Xd = model._upload(X)
        cb = (lambda mdl, state, it: seen.append(AGP.elbo_streamed(mdl, Xd, y, rho=1.0))) if evaluate else None
        AGP.train_(model, X, y, 20, idx_stream=idx, callback=cb)
        runs.append(model.get_state(0))
        assert model._max_batch == S.B
    assert len(seen) == 20 and np.all(np.isfinite(seen))
    errs = [float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(runs[0], runs[1])]
    bitwise = all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    print(f"with / without streamed evaluations: worst relative difference {max(errs):.2e}, bitwise equal: {bitwise}")
    assert max(errs) <= 1e-10


def test_workspace_does_not_grow_with_n(env):
    """free device memory after a streamed call at N = 8229 and after one at N = 5 * 4096 + 1: the only allocation that grows is
    the partial sums, 16 bytes per 256 points, rounded up to the allocator's granularity (2 MiB: the runtime's device-memory pool
    hands out fragments of 2 MiB blocks)"""
    torch, L = env["torch"], env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle("logistic")
    model, twin, Xd, yd = _pair("logistic")
    n2 = 5 * 4096 + 1
    rep = -(-n2 // len(X))
    X2 = torch.cat([Xd] * rep)[:n2].contiguous()
    y2 = torch.cat([yd] * rep)[:n2].contiguous()
    assert _stream(L, model, Xd, yd, len(X))[0] == 0
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    st, v, t = _stream(L, model, X2, y2, n2)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    assert st == 0 and np.isfinite(v)
    gran = 2 << 20
    bound = -(-(16 * -(-n2 // 256)) // gran) * gran
    print(f"free memory {free1} -> {free2}: {free1 - free2} bytes, bound {bound}")
    assert free1 - free2 <= bound
    assert model._max_batch == S.B


def test_fp32(env):
    """yardstick e32: the error of the one-batch fp32 agp_svgp_elbo(fresh_local = 1) against the fp64 oracle on the same inputs
    (the oracle with the reference's Float32 jitter, 1e-3); the streamed fp32 value is within 4 e32 of the oracle"""
    AGP, R, L = env["AGP"], env["R"], env["L"]
    X, y, Z, idx = S.data("logistic", S.NMAX)
    ref = R.SVGP(R.Kernel("sqexponential", S.KSCALE, S.KVAR), R.LogisticLikelihood(), Z, stochastic=True, batchsize=S.B, jitter=1e-3)
    ref.train(X, y, S.STEPS, idx_stream=idx)
    yt = R.treat_labels(y, ref.likelihood)
    want = ref.elbo_fresh(X, yt, 1.0)
    model, twin = S.make_model(AGP, "logistic", T=np.float32), S.make_model(AGP, "logistic", T=np.float32)
    Xd = model._upload(X)
    yd = model._upload_y(model._treat(y))
    v1, t1 = _one_batch(L, twin, Xd, yd, len(X))
    st, v, t = _stream(L, model, Xd, yd, len(X))
    assert st == 0, L.agp_last_error(model._ctx)
    e32, es = abs(v1 - want) / abs(want), abs(v - want) / abs(want)
    print(f"fp32: one-batch error e32 = {e32:.3e}, streamed error = {es:.3e}, ratio {es / e32:.2f}")
    assert es <= 4 * e32


def _refused_handles(env):
    """(name that must appear in the message, model with a live handle, x, y) for every refused handle kind"""
    AGP, L = env["AGP"], env["L"]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 2))
    yb = np.where(X[:, 0] > 0, 1, -1)
    yc = 1 + (np.arange(40) % 3)
    ycount = np.arange(40) % 4
    Z = X[:6].copy()
    k = AGP.SqExponentialKernel()
    svi = lambda: AGP.AnalyticSVI(20)  # noqa: E731
    out = []

    def sparse(name, lik, yy, **kw):
        m = AGP.SVGP(k, lik, kw.pop("inference", None) or svi(), Z, optimiser=False, **kw)
        m._ensure_handle(20)
        out.append((name, m, yy))
        return m

    sparse("Poisson", AGP.PoissonLikelihood(2.0), ycount)
    sparse("Heteroscedastic", AGP.HeteroscedasticLikelihood(1.0), X[:, 1])
    sparse("opt_noise", AGP.GaussianLikelihood(0.1, opt_noise=True), X[:, 1])
    sparse("AGP_FLAG_STALE_K", AGP.LogisticLikelihood(), yb, reference_compat_stale_K=True)
    sparse("latent-sharded", AGP.LogisticSoftMaxLikelihood(3), yc, latent_slice=(0, 2))
    sh = sparse("batch-sharded", AGP.LogisticLikelihood(), yb)
    sh._chk(L.agp_svgp_set_batch_shard(sh._h, 0, 2))
    sparse("AGP_FLAG_NUMERICAL", AGP.LogisticLikelihood(), yb, inference=AGP.QuadratureVI())
    sparse("AGP_FLAG_MC", AGP.LogisticSoftMaxLikelihood(3), yc, inference=AGP.MCIntegrationVI())
    mo = AGP.MOSVGP(k, [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], svi(), [Z, Z], optimiser=False)
    mo._ensure_handle(20)
    out.append(("multi-output", mo, yb))
    vgp = AGP.VGP(X, yb, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    vgp._ensure_handle(0)
    out.append(("AGP_FLAG_FULL", vgp, yb))
    gp = AGP.GP(X, X[:, 1], k, optimiser=False)
    out.append(("AGP_FLAG_EXACT", gp, X[:, 1]))
    mc = AGP.MCGP(X, yb, k, AGP.LogisticLikelihood(), AGP.GibbsSampling())
    mc._ensure_handle(0)
    out.append(("AGP_FLAG_SAMPLED", mc, yb))
    on = AGP.OnlineSVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), AGP.OIPS(0.7), optimiser=False)
    for b in (0, 20):  # the second batch installs the streaming prior
        AGP.train_online(on, X[b:b + 20], yb[b:b + 20], iterations=2)
    out.append(("online", on._cur, yb))
    return X, out


def test_refused_handles_through_the_abi(env):
    torch, L = env["torch"], env["L"]
    X, handles = _refused_handles(env)
    for name, model, yy in handles:
        Xd = torch.as_tensor(X, dtype=model.tdtype, device="cuda")
        yd = torch.as_tensor(np.asarray(yy, dtype=np.float64), dtype=model.tdtype, device="cuda")
        st, v, t = _stream(L, model, Xd, yd, len(X))
        msg = L.agp_last_error(model._ctx).decode()
        assert st == UNSUPPORTED, (name, st, msg)
        assert "agp_svgp_elbo_stream" in msg and name in msg, (name, msg)
        assert v == SENT and t == (SENT, SENT, SENT), name


def test_argument_and_status_paths(env):
    torch, L = env["torch"], env["L"]
    X, y, yt, Z, idx, ref = S.trained_oracle("logistic")
    model, twin, Xd, yd = _pair("logistic")
    n = len(X)
    untouched = (SENT, (SENT, SENT, SENT))
    st, *rest = _stream(L, model, Xd, yd, 0)
    assert st == BAD_BATCH and tuple(rest) == untouched
    st, *rest = _stream(L, model, Xd, yd, n, ldx=S.D - 1)
    assert st == INVALID and tuple(rest) == untouched
    st, *rest = _stream(L, model, Xd, yd, n, rho=0.0)
    assert st == INVALID and tuple(rest) == untouched
    st, *rest = _stream(L, model, Xd, yd, n, rho=-1.0)
    assert st == INVALID and tuple(rest) == untouched
    out = C.c_double(SENT)
    assert L.agp_svgp_elbo_stream(model._h, None, S.D, C.c_void_p(yd.data_ptr()), None, n, 1.0, C.byref(out), None) == INVALID
    assert out.value == SENT
    # terms_host is nullable
    assert L.agp_svgp_elbo_stream(model._h, C.c_void_p(Xd.data_ptr()), S.D, C.c_void_p(yd.data_ptr()), None, n, 1.0, C.byref(out),
                                  None) == 0
    good = out.value
    # a point whose moments are not finite (tests/test_elbo_stream_host.py: no state that agp_svgp_set_state accepts makes var_f
    # negative, and the reference's var_f is not > 0 at exactly this point): the first such point is named, outputs untouched,
    # nothing latched, the handle goes on working.  Point 4353 lies in the second chunk, off the 64- and 256-grids
    bad = Xd.clone()
    for where in (7000, 4353):
        bad[where, 1] = float("nan")
    st, *rest = _stream(L, model, bad, yd, n)
    msg = L.agp_last_error(model._ctx).decode()
    assert st == NEG_KTILDE and tuple(rest) == untouched, (st, msg)
    assert "point 4353 " in msg, msg
    assert L.agp_svgp_check_status(model._h) == 0
    st, v, t = _stream(L, model, Xd, yd, n)
    assert st == 0 and v == good


def test_mirror(env):
    AGP = env["AGP"]
    X, y, yt, Z, idx, ref = S.trained_oracle("studentt")
    model, twin = S.make_model(AGP, "studentt"), S.make_model(AGP, "studentt")
    h0, mb0 = model._h.value, model._max_batch
    a = AGP.ELBO(model, X, y, rho=1.0, streamed=True)
    b = AGP.ELBO(twin, X, y, rho=1.0)
    assert abs(a - b) <= TOL * abs(b)
    assert model._h.value == h0 and model._max_batch == mb0 == S.B
    assert twin._max_batch == len(X)
    # rho = None: the rho left by the last train_ ; idx and return_terms
    v, t = AGP.elbo_streamed(model, X, y, idx=np.arange(len(X))[::-1].copy(), return_terms=True)
    rho = model.inference.rho
    assert rho == len(X) / S.B and abs(v - (rho * t[0] - t[1] - rho * t[2])) <= 1e-12 * abs(v)
    assert abs(v - ref.elbo_fresh(X, yt, rho)) <= TOL * abs(v)
    with pytest.raises(NotImplementedError, match="Poisson"):
        AGP.elbo_streamed(AGP.SVGP(AGP.SqExponentialKernel(), AGP.PoissonLikelihood(2.0), AGP.AnalyticSVI(10), Z, optimiser=False),
                          X, np.arange(len(X)) % 3)
