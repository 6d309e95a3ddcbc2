"""MCGP (Gibbs sampling of the augmented full GP, AGP_FLAG_FULL | AGP_FLAG_SAMPLED) on the MI355X against the NumPy restatement
tests/_mcgp_ref.py: the samplers (agp_sample_local) point by point and against their laws, whole chains, continuation, save / load,
predictions, refusals, and that a chain is enqueued without waiting for the host."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import _mcgp_ref as M
from _liks import agp_lik, oracle_lik

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5
KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel"}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    return dict(AGP=AGP, capi=capi, R=R)


def _model(env, name, nBurnin=0):
    AGP = env["AGP"]
    X, y, likname, kind, scale, mean = M.case_data(name)
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(list(scale))
    k = 1.5 * (getattr(AGP, KERNELS[kind])() @ tr)
    return AGP.MCGP(X, y, k, agp_lik(AGP, likname), AGP.GibbsSampling(nBurnin=nBurnin), mean=mean), X


# ---- the samplers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("likname", ["logistic", "studentt", "negbinomial"])
def test_sample_local_point_by_point(env, likname):
    """every point of a small call against the restatement for the same (seed, t): element-wise arithmetic, relative 1e-12"""
    AGP, R = env["AGP"], env["R"]
    y, f, seed, t = M.local_inputs(likname)
    th, ax = AGP.sample_local(agp_lik(AGP, likname), y, f, seed, t)
    th_r, ax_r = M.sample_local(oracle_lik(R, likname), y, f, seed, t)
    e = np.abs(th - th_r) / np.abs(th_r)
    print(f"{likname}: worst relative error of theta {e.max():.2e}, of aux {np.max(np.abs(ax - ax_r) / np.maximum(np.abs(ax_r), 1e-300)):.2e}")
    assert np.all(e < 1e-12)
    assert np.all(np.abs(ax - ax_r) <= 1e-12 * np.abs(ax_r))


def _z(d, m, s2):
    return (d.mean() - m) / math.sqrt(s2 / len(d))


@pytest.mark.parametrize("c", [0.0, 2.0])
def test_polya_gamma_law_on_the_device(env, c):
    """n = 10^6 draws of PG(1, c): the 5-sigma band on the mean (0.4 % of the mean at c = 0), the KS test against the Gamma series;
    the same call twice is bit-identical, a draw does not depend on the launch's size, another seed or sweep differs"""
    AGP = env["AGP"]
    n = 10 ** 6
    lik, y, f = AGP.LogisticLikelihood(), np.ones(n), np.full(n, c)
    d, ax = AGP.sample_local(lik, y, f, 2024, 3)
    m, s2 = M.pg_moments(1, c)
    D, crit = M.ks_two_sample(d, M.pg1_series(20000, c, np.random.default_rng(8))), M.ks_critical(1e-6, n, 20000)
    print(f"c = {c}: mean z = {_z(d, m, s2):+.2f}, KS D = {D:.4f} (critical {crit:.4f})")
    assert abs(_z(d, m, s2)) < 5.0 and D < crit
    assert np.all(ax == c)
    assert np.array_equal(d, AGP.sample_local(lik, y, f, 2024, 3)[0])
    assert np.array_equal(d[:1000], AGP.sample_local(lik, y[:1000], f[:1000], 2024, 3)[0])
    assert not np.array_equal(d[:1000], AGP.sample_local(lik, y[:1000], f[:1000], 2025, 3)[0])
    assert not np.array_equal(d[:1000], AGP.sample_local(lik, y[:1000], f[:1000], 2024, 4)[0])


def test_polya_gamma_sum_law_on_the_device(env):
    AGP = env["AGP"]
    n = 10 ** 6
    d, _ = AGP.sample_local(AGP.NegBinomialLikelihood(6.0), np.full(n, 4.0), np.full(n, -1.0), 7, 0)  # PG(10, 1)
    m, s2 = M.pg_moments(10, 1.0)
    print(f"PG(10, 1): mean z = {_z(d, m, s2):+.2f}")
    assert abs(_z(d, m, s2)) < 5.0


def test_inverse_gamma_law_on_the_device(env):
    import scipy.stats as st

    AGP = env["AGP"]
    n, nu, sg = 10 ** 6, 8.0, 1.5
    y, f = np.zeros(n), np.full(n, 1.0)
    th, om = AGP.sample_local(AGP.StudentTLikelihood(nu, sg), y, f, 99, 1)
    alpha, beta = 0.5 * (nu + 1.0), 0.5 * (1.0 + sg * sg * nu)
    z = _z(om, beta / (alpha - 1.0), beta ** 2 / ((alpha - 1.0) ** 2 * (alpha - 2.0)))
    D = st.kstest(om, st.invgamma(alpha, scale=beta).cdf).statistic
    print(f"InverseGamma({alpha}, {beta}): mean z = {z:+.2f}, KS D = {D:.5f} (critical {M.ks_critical(1e-6, n):.5f})")
    assert abs(z) < 5.0 and D < M.ks_critical(1e-6, n)
    assert np.array_equal(th, 1.0 / om)


# ---- whole chains ---------------------------------------------------------------------------------------------------------------
CHAIN_TOL = 1e-8  # sweep 1 goes through VGP's factorisation from identical state: VGP's bound; the whole chain is held to the same


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_chain_parity(env, name):
    """20 sweeps: the store, the last f, Sigma and theta against the restatement (relative, max norm).  Prints the error of every
    kept sweep (the series DESIGN.md section 9h quotes)."""
    AGP, capi = env["AGP"], env["capi"]
    model, X = _model(env, name)
    ref, (n, discard, thinning) = M.case_ref(name)
    S = AGP.sample(model, n, discard_initial=discard, thinning=thinning, seed=ref.seed)
    Sr = ref.sample(n, discard, thinning)
    errs = [_rel(S[k], Sr[k]) for k in range(n)]
    print(name, "relative error per kept sweep:", " ".join(f"{e:.1e}" for e in errs))
    assert model.sweep_counter() == ref.t == 20 and model.inference.n_iter == 20
    if discard == 0:
        assert errs[0] < 1e-8
    assert max(errs) < CHAIN_TOL
    f, Sig = model.get_state()
    assert np.array_equal(f, S[-1])
    assert _rel(Sig, ref.Sigma) < CHAIN_TOL
    assert _rel(model.get_matrix(capi.VEC_THETA, 0, len(X)), ref.theta) < CHAIN_TOL
    assert np.array_equal(model.inference.sample_store, S)


def test_initial_state(env):
    model, X = _model(env, "logistic-173")
    f, Sig = model.get_state()
    assert np.array_equal(f, np.zeros(len(X))) and np.array_equal(Sig, np.eye(len(X)))  # latentgp.jl:81-86
    assert model.sweep_counter() == 0


@pytest.mark.parametrize("name", ["logistic-200", "studentt-173", "negbinomial-173"])
def test_continuation_is_bitwise(env, name, tmp_path):
    """sample(10) twice equals sample(20) once, bit for bit (cat = true); a saved and reloaded model continues identically"""
    AGP = env["AGP"]
    one, _ = _model(env, name)
    two, _ = _model(env, name)
    S = AGP.sample(one, 20, seed=5)
    a = AGP.sample(two, 10, seed=5)
    AGP.save_trained_model(str(tmp_path / "mcgp"), two)
    b = AGP.sample(two, 10)
    assert np.array_equal(np.concatenate([a, b]), S) and np.array_equal(two.inference.sample_store, S)
    assert two.sweep_counter() == 20 and two.seed == 5
    three = AGP.load_trained_model(str(tmp_path / "mcgp"))
    assert isinstance(three, AGP.MCGP) and three.seed == 5 and three.sweep_counter() == 10
    assert np.array_equal(three.inference.sample_store, a) and np.array_equal(three.get_state()[0], a[-1])
    assert np.array_equal(AGP.sample(three, 10), b) and np.array_equal(three.inference.sample_store, S)
    c = AGP.sample(two, 3, cat=False)
    assert np.array_equal(two.inference.sample_store, c) and two.sweep_counter() == 23


def test_seed_is_drawn_and_recorded(env):
    AGP = env["AGP"]
    m1, _ = _model(env, "logistic-173")
    m2, _ = _model(env, "logistic-173")
    a, b = AGP.sample(m1, 2), AGP.sample(m2, 2, seed=m1.seed + 1)
    assert m1.seed is not None and not np.array_equal(a, b)
    m3, _ = _model(env, "logistic-173")
    assert np.array_equal(AGP.sample(m3, 2, seed=m1.seed), a)


# ---- predictions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nt", [("logistic-173", 300), ("studentt-200", 300), ("negbinomial-173", 300), ("logistic-200", 4096 + 37)])
def test_predictions(env, name, nt):
    """predict_f (mean; mean and variance), predict_y, proba_y on a 50-sample store against the restatement on the device's own
    samples: 1e-8, variances 1e-6 (as for VGP); 4096 + 37 test points cross one block of the prediction workspace"""
    AGP = env["AGP"]
    model, X = _model(env, name)
    ref, _ = M.case_ref(name)
    S = AGP.sample(model, 50, discard_initial=5, seed=3)
    Xt = np.random.default_rng(4).random((nt, 3))
    mu_r, var_r = ref.predict_f(Xt, S)
    mu = AGP.predict_f(model, Xt)
    mu2, var = AGP.predict_f(model, Xt, cov=True)
    print(f"{name}: mean {_rel(mu, mu_r):.1e}  variance {_rel(var, var_r):.1e}")
    assert _rel(mu, mu_r) < 1e-8 and np.array_equal(mu, mu2)
    assert _rel(var, var_r) < 1e-6
    with pytest.raises(NotImplementedError):
        AGP.predict_f(model, Xt, cov=True, diag=False)
    py = AGP.predict_y(model, Xt)
    lik = ref.lik.name
    if lik == "logistic":
        assert np.array_equal(py, mu > 0)
        p, pv = AGP.proba_y(model, Xt)
        p_r, pv_r = ref.proba_y_logistic(Xt, S)
        assert _rel(p, p_r) < 1e-8 and _rel(pv, pv_r) < 1e-6
    elif lik == "studentt":
        assert np.array_equal(py, mu)
        p, pv = AGP.proba_y(model, Xt)  # (beyond the reference: compute_proba on the moments, studentt.jl:57-61)
        assert np.array_equal(p, mu) and _rel(pv, np.maximum(var_r, 0) + 3.0 * 1.0 / (3.0 - 2.0)) < 1e-6
    else:
        pn = 1.0 / (1.0 + np.exp(mu_r))
        assert _rel(py, 6.0 * (1.0 - pn) / pn) < 1e-8
        # (beyond the reference: compute_proba of the likelihood on the moments, negativebinomial.jl:45-60 -- mean and variance of
        #  r sigma(f) / (1 - sigma(f)) under N(mu, var) by the 100-node Gauss-Hermite rule of predictions.jl:4)
        p, pv = AGP.proba_y(model, Xt)
        gx, gw = np.polynomial.hermite.hermgauss(100)
        xq = gx[None, :] * math.sqrt(2.0) * np.sqrt(np.maximum(var_r, 0.0))[:, None] + mu_r[:, None]
        vq = 6.0 * np.exp(xq)  # r sigma / (1 - sigma) = r exp(f)
        p_r = vq @ (gw / math.sqrt(math.pi))
        pv_r = (vq * vq) @ (gw / math.sqrt(math.pi)) - p_r * p_r
        print(f"{name}: proba_y mean {_rel(p, p_r):.1e}  variance {_rel(pv, pv_r):.1e}")
        assert _rel(p, p_r) < 1e-8 and _rel(pv, pv_r) < 1e-6


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    from test_gpu_vgp import create_status

    AGP, capi = env["AGP"], env["capi"]
    L = capi.lib()
    FS = capi.FLAG_FULL | capi.FLAG_SAMPLED
    lik = lambda kind, p0=0.0, p1=0.0, nc=1: capi.LikDesc(kind, nc, p0, p1)
    cases = [(dict(flags=FS, lik=lik(capi.LIK_GAUSSIAN, 0.05)), 5, "For a Gaussian Likelihood you should directly use the `GP` model"),
             (dict(flags=FS, lik=lik(capi.LIK_LAPLACE, 0.4)), 5, "Logistic, StudentT and NegBinomial"),
             (dict(flags=FS, lik=lik(capi.LIK_BAYESIANSVM)), 5, "Logistic, StudentT and NegBinomial"),
             (dict(flags=FS, lik=lik(capi.LIK_POISSON, 2.0)), 5, "Logistic, StudentT and NegBinomial"),
             (dict(flags=FS, lik=lik(capi.LIK_NEGBINOMIAL, 2.5)), 1, "r must be an integer"),
             (dict(flags=FS | capi.FLAG_EXACT), 5, "Logistic, StudentT and NegBinomial"),
             (dict(flags=capi.FLAG_SAMPLED), 5, "Gibbs sampling runs on the full model"),
             (dict(flags=FS, dtype=capi.F32), 5, "Float64 only"),
             (dict(flags=FS), 0, "")]
    for fields, status, msg in cases:
        st, err = create_status(capi, **fields)
        assert st == status and msg in err, (fields, st, err)
    model, X = _model(env, "logistic-173")
    N = len(X)
    AGP.sample(model, 2, seed=1)
    h, ctx = model._h, model._ctx
    Xd, yd, _ = model._data
    out, o3 = C.c_double(), (C.c_double * 3)()

    def refused(st, what):
        assert st == UNSUPPORTED and what in L.agp_last_error(ctx).decode(), (st, L.agp_last_error(ctx))

    refused(L.agp_svgp_cavi_step(h, C.c_void_p(Xd.data_ptr()), 3, C.c_void_p(yd.data_ptr()), None, N, 1.0), "agp_svgp_cavi_step")
    refused(L.agp_svgp_elbo(h, C.c_void_p(Xd.data_ptr()), 3, C.c_void_p(yd.data_ptr()), None, N, 1.0, 0, C.byref(out)), "agp_svgp_elbo")
    refused(L.agp_svgp_elbo_terms(h, o3), "agp_svgp_elbo_terms")
    refused(L.agp_svgp_hyper_step(h), "agp_svgp_hyper_step")
    refused(L.agp_svgp_hypergrad(h, 0, C.byref(out), o3, None), "agp_svgp_hypergrad")
    refused(L.agp_svgp_predict_f(h, C.c_void_p(Xd.data_ptr()), 3, 5, C.c_void_p(yd.data_ptr()), None), "agp_svgp_predict_f")
    refused(L.agp_svgp_get_state(h, 0, None, None, C.c_void_p(yd.data_ptr()), None), "eta1 / eta2 must be NULL")
    assert L.agp_svgp_step_local(h, None, 3, None, None, N, 1.0) == UNSUPPORTED
    assert L.agp_svgp_cavi_step_multi(h, None, 0, None, 3, None, None, N, 1.0) == UNSUPPORTED
    # a handle that is not sampled refuses the new entry points; the chain's arguments are checked
    vgp = AGP.VGP(X, (X[:, 0] > 0.5).astype(int), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(vgp, 1)
    t = C.c_int64()
    assert L.agp_svgp_gibbs_counter(vgp._h, 0, C.byref(t)) == UNSUPPORTED
    assert L.agp_svgp_gibbs_sample(vgp._h, C.c_void_p(yd.data_ptr()), 1, 0, 1, 0, C.c_void_p(Xd.data_ptr()), N) == UNSUPPORTED
    assert L.agp_svgp_gibbs_sample(h, C.c_void_p(yd.data_ptr()), 1, 0, 0, 0, C.c_void_p(Xd.data_ptr()), N) == 1
    assert L.agp_svgp_predict_samples(h, C.c_void_p(Xd.data_ptr()), 3, 5, C.c_void_p(Xd.data_ptr()), N, 2, 3, C.c_void_p(yd.data_ptr()),
                                      C.c_void_p(yd.data_ptr())) == 1
    assert "mode 0, 1 or 2" in L.agp_last_error(ctx).decode()
    with pytest.raises(capi.AGPError, match="Logistic, StudentT and NegBinomial"):
        AGP.sample_local(AGP.LaplaceLikelihood(0.4), np.zeros(4), np.zeros(4), 1)
    for bad in (-1.0, 2.5):  # a NegBinomial target that is no non-negative integer: latched, AGP_ERR_LABELS
        with pytest.raises(capi.AGPError, match="AGP_ERR_LABELS.*non-negative integers"):
            AGP.sample_local(AGP.NegBinomialLikelihood(6.0), np.array([3.0, bad, 0.0]), np.zeros(3), 1)
    st_big = L.agp_svgp_predict_samples(h, C.c_void_p(Xd.data_ptr()), 3, 5, C.c_void_p(Xd.data_ptr()), N, 65537, 0,
                                        C.c_void_p(yd.data_ptr()), None)
    assert st_big == 1 and "at most 65536 samples" in L.agp_last_error(ctx).decode()
    st_model, _ = _model(env, "studentt-173")
    AGP.sample(st_model, 2, seed=1)
    S = st_model._store_dev()
    refused_st = L.agp_svgp_predict_samples(st_model._h, C.c_void_p(Xd.data_ptr()), 3, 5, C.c_void_p(S.data_ptr()), N, 2, 2,
                                            C.c_void_p(yd.data_ptr()), C.c_void_p(yd.data_ptr()))
    assert refused_st == UNSUPPORTED and "Bernoulli" in L.agp_last_error(st_model._ctx).decode()
    assert model.sweep_counter() == 2  # nothing above advanced the chain


# ---- no host synchronisation inside a chain ---------------------------------------------------------------------------------------
def test_chain_is_enqueued_ahead_of_the_device(env):
    """agp_svgp_gibbs_sample returns while the chain still runs, after less host time than half the chain's device time (HIP events
    around the call): had any sweep waited for the host, the call could not return before the sweeps before it had finished"""
    import torch

    AGP, capi = env["AGP"], env["capi"]
    L = capi.lib()
    N, S = 2048, 60
    rng = np.random.default_rng(1)
    X = rng.random((N, 4))
    y = (np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 > 0).astype(int)
    model = AGP.MCGP(X, y, 1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0)), AGP.LogisticLikelihood(), AGP.GibbsSampling(nBurnin=0))
    AGP.sample(model, 2, seed=9)  # (the first call refreshes K and synchronises once; allocations)
    yd = model._data[1]
    store = torch.empty(1, N, dtype=torch.float64, device=model._dev())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    st = L.agp_svgp_gibbs_sample(model._h, C.c_void_p(yd.data_ptr()), 1, S - 1, 1, C.c_uint64(9), C.c_void_p(store.data_ptr()), N)
    host_ms = 1e3 * (time.perf_counter() - t0)
    e1.record()
    still_running = not e1.query()
    assert st == 0
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1)
    print(f"{S} sweeps at N = {N}: host {host_ms:.2f} ms to enqueue, device {dev_ms:.2f} ms ({dev_ms / S:.3f} ms per sweep); "
          f"still running at return: {still_running}")
    assert L.agp_svgp_check_status(model._h) == 0
    assert still_running and host_ms < 0.5 * dev_ms
