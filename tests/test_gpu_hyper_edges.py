"""GPU: the hyper-gradient kernels (agp_hyper.h) at the dimension, tile and type edges of tests/_hyper_cases.py.

Every other test takes a device hyper-gradient at D <= 4.  The backward pass through the kernel matrix (kernel_backward_body behind
k_kernel_backward / k_kernel_backward2, reduced by k_hyper_reduce*) stages 32 input dimensions at a time: one chunk up to D = 32,
two up to D = 64 = HB_MAXD, refusal above.  Here the gradient is taken at D = 1, 31, 32, 33, 64 with m and B on and off the 64-grid,

* against torch.autograd of the objective restated in tests/_torch_elbo.py, evaluated at the DEVICE'S OWN mu, Sigma and theta (nothing
  of the oracle enters): 1e-7, the bound of test_device_hyper_gradient_is_what_autograd_gives;
* against R.hyper_gradient of the oracle trained on the same index stream: 1e-8, the bound of test_hypergrad_matches_oracle;
* in float32 against the float64 oracle: 2e-2 of the largest entry, the bound of test_fp32_hyper_gradient_and_multiclass;
* on the full model (k_vgp_gK, X on both sides) against _torch_elbo.neg_kl_hypergrad at the 1e-6 of test_vgp_hypergrad_kernels;
dscale is compared per dimension and dZ per entry, each relative to the vector's largest reference entry
(tests/test_hyper_edges_host.py shows that no dimension's column of dZ is below 0.05 of that), dvariance relative to max(1, |.|).
Plus: the gradient inside agp_svgp_hyper_step with G_K from the fused product (read back from a Descent step), twice the same
gradient bit for bit, and D = 65 refused with nothing written and the handle still usable."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _knobs as KN

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hyper_cases as HC  # noqa: E402

JITTER = 1e-4  # the reference's constant for Float64 (src/functions/utils.jl:8-9), the library's default
UNSUPPORTED = 5


@pytest.fixture(scope="module")
def mods(built):
    import torch

    assert torch.cuda.is_available()
    import agp_amd as AGP
    from agp_amd import capi

    from oracle import agp_ref as R

    return AGP, R, capi, torch


def _train(mods, c, optimiser=False, iters=HC.ITERS):
    AGP = mods[0]
    X, y, Z, sc, idx = HC.make_inputs(c)
    ma = AGP.SVGP(HC.device_kernel(AGP, c["kind"], c["transform"], sc), HC.device_lik(AGP, c), AGP.AnalyticSVI(c["B"]), np.array(Z),
                  optimiser=optimiser, elbo_mode=c["mode"], T=np.float32 if c["f32"] else np.float64)
    AGP.train_(ma, np.array(X), np.array(y), iters, idx_stream=idx[:iters])
    return ma


def _counters(ma, capi):
    ng, nf = C.c_int64(), C.c_int64()
    ma._chk(capi.lib().agp_svgp_hyper_counters(ma._h, C.byref(ng), C.byref(nf)))
    return ng.value, nf.value


@pytest.mark.parametrize("c", HC.CASES, ids=HC.case_id)
def test_hyper_gradient_at_dimension_and_tile_edges(mods, c):
    import _torch_elbo as TE

    AGP, R, capi, torch = mods
    X, y, Z, sc, idx = HC.make_inputs(c)
    D, m, B = c["D"], c["m"], c["B"]
    ma = _train(mods, c)
    assert ma.n_latent == {"heteroscedastic": 2, "logisticsoftmax": 3}.get(c["lik"], 1)
    got = [ma.hypergrad(k) for k in range(ma.n_latent)]
    for dv, ds, dz in got:
        assert ds.shape == (D,) and dz.shape == (m, D)  # all D entries, also for a ScaleTransform and for no transform
    ng, nf = _counters(ma, capi)
    assert ng == ma.n_latent
    # agp_svgp_hypergrad first takes the pending natural-gradient step with the stand-alone kernel, so its G_K never comes from the
    # one product C (Sigma K^-1): that form belongs to agp_svgp_hyper_step (test_fused_gradient_of_the_hyper_step below)
    assert nf == 0
    worst_a = None
    if c["lik"] in HC.RESTATED:
        mu, Sig, _, _ = ma.get_state(0)
        yt = np.asarray(ma._treat(np.array(y)), dtype=np.float64)
        local = {} if c["lik"] == "gaussian" else {"theta": ma.get_matrix(capi.VEC_THETA, 0)}
        last = idx[HC.ITERS - 1]
        a = TE.autograd_hypergrad(c["kind"], HC.restated_lik(c), X[last], yt[last], Z, sc, HC.VARIANCE, mu, Sig, np.zeros(m), local,
                                  len(X) / B, JITTER, c["mode"])
        worst_a = HC.errors(got[0], a[:3])
    _, _, _, _, grads = HC.oracle_run(c, R)
    worst_o = [HC.errors(got[k], (g["dvariance"], g["dscale"], g["dZ"])) for k, g in enumerate(grads)]
    fmt = lambda e: "dvariance %.1e dscale %.1e dZ %.1e" % tuple(e)
    print(f"{HC.case_id(c)}: fused G_K {nf}/{ng}; vs autograd at the device's state: {fmt(worst_a) if worst_a else 'no restatement'}; "
          f"vs oracle: {' | '.join(fmt(e) for e in worst_o)}")
    if worst_a is not None:
        assert HC.within(worst_a, 1e-7), worst_a
    for e in worst_o:
        assert HC.within(e, 1e-8), e


FUSED_ETA = 1e-3


@pytest.mark.parametrize("c", [c for c in HC.CASES if c["shape"] == "d64f"], ids=HC.case_id)
def test_fused_gradient_of_the_hyper_step(mods, c):
    """D = 64, m = 192, B = 256: inside train_ the hyper step finds the natural-gradient step still pending, the factorisation launch
    takes it as its prologue and leaves C = kappa' diag(w) kappa + K^-1 / 4 behind, and G_K is the one product C (Sigma K^-1)
    (k_hyper_gK_fused; the counters say so).  That gradient never leaves the device as such: the step is taken with
    Descent(eta) on the kernel parameters (in log space: log p += eta p dp) and on Z (Z += eta dZ), five iterations hold exactly one
    hyper step (after the fourth), and the gradient is read back from what moved -- to eps / (eta |g|) ~ 1e-12 of its largest entry
    -- and compared with R.hyper_gradient of the oracle after four steps at 1e-8."""
    AGP, R, capi, torch = mods
    X, y, Z, sc, idx = HC.make_inputs(c)
    assert c["transform"] == "ard" and len(idx) == 5
    ma = AGP.SVGP(HC.device_kernel(AGP, c["kind"], c["transform"], sc), HC.device_lik(AGP, c), AGP.AnalyticSVI(c["B"]), np.array(Z),
                  optimiser=AGP.Descent(FUSED_ETA), Zoptimiser=AGP.Descent(FUSED_ETA))
    AGP.train_(ma, np.array(X), np.array(y), 5, idx_stream=idx)
    ng, nf = _counters(ma, capi)
    assert ng == 1, ng
    if not (KN.no_prologue() or KN.forced("AGP_HYPER_GK_FUSED")):
        assert nf == 1, (ng, nf)
    k = ma.kernels[0]
    got = (np.log(k.variance / HC.VARIANCE) / (FUSED_ETA * HC.VARIANCE), np.log(k.transform.v / sc) / (FUSED_ETA * sc),
           (ma.Zs[0] - Z) / FUSED_ETA)
    g = HC.oracle_run(c, R, iters=4)[4][0]
    e = HC.errors(got, (g["dvariance"], g["dscale"], g["dZ"]))
    print(f"{HC.case_id(c)}: fused G_K {nf}/{ng}; gradient of the hyper step vs oracle: dvariance {e[0]:.1e} dscale {e[1]:.1e} "
          f"dZ {e[2]:.1e}")
    assert HC.within(e, 1e-8), e


@pytest.mark.parametrize("c", HC.F32_CASES, ids=HC.case_id)
def test_float32_hyper_gradient_at_two_chunks(mods, c):
    AGP, R, capi, torch = mods
    ma = _train(mods, c)
    got = ma.hypergrad(0)
    g = HC.oracle_run(c, R)[4][0]  # float64, jitter 1e-3
    e = HC.errors(got, (g["dvariance"], g["dscale"], g["dZ"]))
    print(f"{HC.case_id(c)}: float32 vs the float64 oracle: dvariance {e[0]:.1e} dscale {e[1]:.1e} dZ {e[2]:.1e}")
    assert HC.within(e, 2e-2), e


@pytest.mark.parametrize("D,N,kind,transform", HC.VGP_CASES, ids=lambda v: str(v))
def test_full_model_hyper_gradient_at_dimension_edges(mods, D, N, kind, transform):
    """VGP(...).hypergrad(0): G_K from k_vgp_gK, one backward pass with X on both sides, k_hyper_reduce -- as _hypergrad_vs_autograd
    of tests/test_gpu_vgp_edges.py, at its tolerance, and every one of the D entries of dscale on its own."""
    from _torch_elbo import neg_kl_hypergrad

    AGP, R, capi, torch = mods
    X, y, sc = HC.vgp_inputs(D, N, transform)
    model = AGP.VGP(X, y, HC.device_kernel(AGP, kind, transform, sc), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(model, HC.ITERS)
    dv, ds = model.hypergrad(0)
    mu, Sig, _, _ = model.get_state(0)
    av, as_ = neg_kl_hypergrad(kind, X, sc, HC.VARIANCE, mu, np.zeros(N), Sig)
    es = HC.max_error(ds, as_)
    print(f"VGP D={D} N={N} {kind} {transform}: dvariance {abs(dv - av) / abs(av):.1e} dscale {es:.1e}")
    assert ds.shape == (D,)
    assert dv == pytest.approx(av, rel=1e-6)
    assert es < 1e-6, (ds, as_)
    if transform == "scale":  # a ScaleTransform's single parameter receives the sum
        assert float(np.sum(ds)) == pytest.approx(float(np.sum(as_)), rel=1e-6)


def test_hyper_gradient_twice_is_bit_identical(mods):
    """the two-stage reduction is deterministic: the same state, two evaluations, the same bits (D = 33, m = 130, B = 129)"""
    c = next(c for c in HC.CASES if c["shape"] == "d33" and c["transform"] == "ard" and c["lik"] == "logistic")
    ma = _train(mods, c)
    a, b = ma.hypergrad(0), ma.hypergrad(0)
    assert np.isfinite(a[0]) and np.all(np.isfinite(a[1])) and np.all(np.isfinite(a[2])) and np.max(np.abs(a[2])) > 0
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- D = 65: above HB_MAXD.  hyper_alloc() refuses before any launch: no kernel of the backward pass runs -------------------------
SENTINEL = -7.25


def _refused(model, capi, dZ, z_opt):
    """agp_svgp_hypergrad and agp_svgp_hyper_step on a handle at D = 65 -> AGP_ERR_UNSUPPORTED, the message names the limit, and the
    outputs keep their bits"""
    L, h, D = capi.lib(), model._h, model.D
    dv, ds = C.c_double(SENTINEL), (C.c_double * D)(*([SENTINEL] * D))
    st = L.agp_svgp_hypergrad(h, 0, C.byref(dv), ds, None if dZ is None else C.c_void_p(dZ.data_ptr()))
    msg = L.agp_last_error(model._ctx).decode()
    assert st == UNSUPPORTED, (st, msg)
    assert "64" in msg and "dimension" in msg, msg
    assert dv.value == SENTINEL and all(v == SENTINEL for v in ds)
    model._chk(L.agp_svgp_hyper_configure(h, 1, 0.01, 1 if z_opt else 0, 0.001 if z_opt else 0.0, 0.9, 0.999, 1e-8))
    st = L.agp_svgp_hyper_step(h)
    msg = L.agp_last_error(model._ctx).decode()
    model._chk(L.agp_svgp_hyper_configure(h, 0, 0.0, 0, 0.0, 0.9, 0.999, 1e-8))
    assert st == UNSUPPORTED, (st, msg)
    assert "64" in msg and "dimension" in msg, msg
    if dZ is not None:
        model._chk(L.agp_ctx_sync(model._ctx))
        assert bool((dZ == SENTINEL).all())


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


def test_sparse_hyper_gradient_above_64_dimensions_is_refused(mods):
    AGP, R, capi, torch = mods
    c = HC.refused_case()
    assert c["D"] == 65
    X, y, Z, sc, idx = HC.make_inputs(c)
    ma = _train(mods, c, iters=1)
    dZ = torch.full((c["m"], c["D"]), SENTINEL, dtype=torch.float64, device="cuda")
    _refused(ma, capi, dZ, z_opt=True)
    # the handle is still usable: a further step lands where the oracle's second step lands
    AGP.train_(ma, np.array(X), np.array(y), 1, idx_stream=idx[1:2], state=True)
    lik = HC.oracle_lik(R, c)
    mr = R.SVGP(R.Kernel(c["kind"], np.array(sc), HC.VARIANCE), lik, np.array(Z), stochastic=True, batchsize=c["B"])
    mr.train(np.array(X), np.array(y), 2, idx_stream=idx[:2])
    mu, Sig, e1, e2 = ma.get_state(0)
    print(f"D = 65 sparse, step after the refusal: eta1 {_rel(e1, mr.latents[0].eta1):.1e} eta2 {_rel(e2, mr.latents[0].eta2):.1e}")
    assert _rel(e1, mr.latents[0].eta1) < 1e-9 and _rel(e2, mr.latents[0].eta2) < 1e-8
    # the Python class with an optimiser: the library's refusal surfaces at the first hyper step of train_
    mo = AGP.SVGP(HC.device_kernel(AGP, c["kind"], c["transform"], sc), HC.device_lik(AGP, c), AGP.AnalyticSVI(c["B"]), np.array(Z),
                  optimiser=AGP.ADAM(0.01))
    rng = np.random.default_rng(1)
    with pytest.raises(capi.AGPError, match="above the supported maximum of 64") as ei:
        AGP.train_(mo, np.array(X), np.array(y), 6, idx_stream=[rng.choice(len(X), c["B"], replace=False) for _ in range(6)])
    assert ei.value.status == UNSUPPORTED


def test_full_model_hyper_gradient_above_64_dimensions_is_refused(mods):
    from _vgp_ref import VGPRef

    AGP, R, capi, torch = mods
    D, N = 65, 65
    X, y, sc = HC.vgp_inputs(D, N, "ard")
    kern = lambda: HC.device_kernel(AGP, "sqexponential", "ard", sc)
    model = AGP.VGP(X, y, kern(), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(model, 1)
    _refused(model, capi, None, z_opt=False)
    # (with a dZ buffer a full model refuses already because its inputs are not optimised: the buffer keeps its bits all the same)
    dZ = torch.full((N, D), SENTINEL, dtype=torch.float64, device="cuda")
    dv, ds = C.c_double(SENTINEL), (C.c_double * D)(*([SENTINEL] * D))
    assert capi.lib().agp_svgp_hypergrad(model._h, 0, C.byref(dv), ds, C.c_void_p(dZ.data_ptr())) == UNSUPPORTED
    model._chk(capi.lib().agp_ctx_sync(model._ctx))
    assert bool((dZ == SENTINEL).all()) and dv.value == SENTINEL and all(v == SENTINEL for v in ds)
    AGP.train_(model, 1, state=True)
    lik = R.LogisticLikelihood()
    ref = VGPRef(R.Kernel("sqexponential", np.array(sc), HC.VARIANCE), lik, X)
    yt = R.treat_labels(y, lik)
    ref.step(yt)
    ref.step(yt)
    mu, Sig, e1, e2 = model.get_state(0)
    print(f"D = 65 full, step after the refusal: eta1 {_rel(e1, ref.eta1[0]):.1e} eta2 {_rel(e2, ref.eta2[0]):.1e}")
    assert _rel(e1, ref.eta1[0]) < 1e-9 and _rel(e2, ref.eta2[0]) < 1e-8
    # VGP's default optimiser is ADAM(0.01): at D = 65 the first hyper step of train_ raises the library's message
    mo = AGP.VGP(X, y, kern(), AGP.LogisticLikelihood(), AGP.AnalyticVI())
    with pytest.raises(capi.AGPError, match="above the supported maximum of 64") as ei:
        AGP.train_(mo, 6)
    assert ei.value.status == UNSUPPORTED
