"""VGP on the MI355X against tests/_vgp_ref.py where the device path changes: the Cholesky driver (nt = mp / 64: single tile, task
graph, per column, blocked), kernels other than SE with a scalar scale, prior means, hyper steps on every latent, and the in-stream
fallback of a factorisation that lost a task-graph dependency."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_vgp import _case, _check_state, _rel, env  # noqa: F401  (env: the module's fixture)

pytestmark = pytest.mark.gpu

ARD = [1.5, 2.5, 1.0]


def _run(env, model, ref, yt, checkpoints):
    """train both to each checkpoint (iterations counted from the start) and compare state, local variables and ELBO there"""
    AGP, done = env["AGP"], 0
    for it in checkpoints:
        AGP.train_(model, it - done, state=None if done == 0 else True)
        for _ in range(it - done):
            ref.step(yt)
        done = it
        _check_state(env, model, ref, yt)


def _var_tol(ref, k, Xt, var):
    """bound on the relative disagreement of predictive variances.  var* = k** + jitt - ks' A ks, A = K^-1 - K^-1 Sigma K^-1, cancels
    terms of size S = max_i |ks_i|' |A| |ks_i|, and each side's A carries a rounding of ~eps cond(K) relative to its entries (both
    form K^-1 explicitly), so the two agree to about eps cond_1(K + 1e-4 I) S in absolute terms.  1e-6 (the tolerance of
    test_vgp_predictions) where that is smaller: N <= a few hundred.  Measured with this data: N = 2049 cond ~ 1.5e8, S ~ 1e3, bound
    2.7e-4 relative to max var*, observed 1.3e-5; N = 6017 cond ~ 5.8e8, S ~ 3.3e3, observed 4.2e-5.  A posterior or a solve that
    is wrong rather than rounded moves var* by O(1)."""
    Ks = ref.kernels[k].matrix(Xt, ref.X)
    Kinv = ref.Kinvs[k]
    A = Kinv - Kinv @ ref.Sigma[k] @ Kinv
    S = np.max(np.einsum("ij,jk,ik->i", np.abs(Ks), np.abs(A), np.abs(Ks)))
    cond = np.max(np.sum(np.abs(ref.Ks[k]), axis=0)) * np.max(np.sum(np.abs(Kinv), axis=0))
    return max(1e-6, np.finfo(np.float64).eps * cond * S / np.max(np.abs(var)))


def _check_predictions(env, model, ref, Xt, proba=True):
    from oracle import agp_ref as R

    AGP = env["AGP"]
    mus, vars_, _ = ref.predict_f(Xt)
    mf, vf = AGP.predict_f(model, Xt, cov=True)
    if model.n_latent == 1:
        mf, vf = [mf], [vf]
    for k in range(model.n_latent):
        assert _rel(mf[k], mus[k]) < 1e-8
        assert _rel(vf[k], vars_[k]) < _var_tol(ref, k, Xt, vars_[k])
    if not proba:
        return
    pa = AGP.proba_y(model, Xt)
    pr = R.compute_proba(ref.lik, tuple(mus), tuple(vars_))
    if ref.lik.name == "logisticsoftmax":
        for k, p in enumerate(pa.values()):
            assert _rel(p, pr[:, k]) < 1e-8
    else:
        # (p = E sigma(f), f ~ N(mu*, var*): |dp / dvar*| <= max|sigma''| / 2 < 0.05, so p inherits 0.05 x the variances' bound)
        vtol = _var_tol(ref, 0, Xt, vars_[0])
        ptol = max(1e-8, 0.05 * vtol * np.max(np.abs(vars_[0])) / np.max(np.abs(pr[0]))) if ref.lik.name != "heteroscedastic" else 1e-8
        assert _rel(pa[0], pr[0]) < ptol and _rel(pa[1], pr[1]) < vtol


# ---- a. tile edges and driver boundaries --------------------------------------------------------------------------------------
# N <= 64: one tile, the task graph's single-tile write_x path; 65: two tiles; 2049: the first size factored by one launch per column
EDGES = ([(N, lik) for N in (2, 63, 64, 65) for lik in ("logistic", "heteroscedastic")]
         + [(N, "logisticsoftmax") for N in (63, 64, 65)] + [(2049, "logistic"), (2049, "logisticsoftmax")])


@pytest.mark.parametrize("N,likname", EDGES)
def test_vgp_tile_edges(env, N, likname):
    X, yt, model, ref = _case(env, likname, N, seed=5)
    if likname == "logisticsoftmax":
        assert np.all(np.sum(yt, axis=0) > 0)  # every class has points
    _run(env, model, ref, yt, (1, 2, 5))
    if N in (64, 2049):
        Xt = np.random.default_rng(N).random((57, 3))
        _check_predictions(env, model, ref, Xt)


# ---- b. blocked factorisation -------------------------------------------------------------------------------------------------
# 6017: nt = 95, La = -2 eta2 is factored with its eta1 extension row by the blocked driver (nt + 1 = 96), K per column;
# 6150: nt = 97, both blocked, the last column group holds one column, trtri_levels at an odd nt
@pytest.mark.parametrize("N", [6017, 6150])
def test_vgp_blocked(env, N):
    AGP = env["AGP"]
    X, yt, model, ref = _case(env, "logistic", N, seed=5)
    AGP.train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    # 1-norm estimate of cond(K + 1e-4 I) from the restatement's own inverse (~5.8e8 and ~5.9e8 here, 1.5e8 at N = 2049): state and
    # ELBO parity hold at 1e-8 as at N = 4100; the predictive variances take the bound _var_tol derives from it
    cond = np.max(np.sum(np.abs(ref.K), axis=0)) * np.max(np.sum(np.abs(ref.Kinv), axis=0))
    assert cond < 1e9, cond
    _check_state(env, model, ref, yt)
    Xt = np.random.default_rng(2).random((64, 3))
    _check_predictions(env, model, ref, Xt, proba=False)


# ---- c. kernels ---------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [("matern52", 2.0), ("matern32", 2.0), ("exponential", 2.0), ("sqexponential", ARD), ("matern52", ARD)]


@pytest.mark.parametrize("likname", ["logistic", "poisson"])
@pytest.mark.parametrize("kind,scale", KERNEL_CASES, ids=lambda v: "ard" if isinstance(v, list) else str(v))
def test_vgp_kernels(env, likname, kind, scale):
    X, yt, model, ref = _case(env, likname, 150, kind=kind, scale=scale)
    _run(env, model, ref, yt, (1, 4))
    _check_predictions(env, model, ref, np.random.default_rng(1).random((57, 3)))


def _hypergrad_vs_autograd(env, model, kind, scale, X, mu0):
    from _torch_elbo import neg_kl_hypergrad

    dv, ds = model.hypergrad(0)
    mu, Sig, _, _ = model.get_state(0)
    av, as_ = neg_kl_hypergrad(kind, X, scale, 1.5, mu, mu0, Sig)
    # (both sides sum products of K^-1's O(cond K) entries into an O(1) gradient: agreement to 1e-6 of the result)
    assert dv == pytest.approx(av, rel=1e-6)
    if np.isscalar(scale):
        assert float(np.sum(ds)) == pytest.approx(float(np.sum(as_)), rel=1e-6)
    else:
        assert np.max(np.abs(ds - as_)) < 1e-6 * np.max(np.abs(as_)), (ds, as_)


@pytest.mark.parametrize("kind", ["sqexponential", "matern52", "matern32"])
@pytest.mark.parametrize("scale", [2.0, ARD], ids=["scalar", "ard"])
def test_vgp_hypergrad_kernels(env, kind, scale):
    X, yt, model, ref = _case(env, "logistic", 120, kind=kind, scale=scale)
    env["AGP"].train_(model, 3)
    _hypergrad_vs_autograd(env, model, kind, scale, X, np.zeros(len(X)))


def test_vgp_hypergrad_exponential_is_refused(env):
    capi = env["capi"]
    X, yt, model, ref = _case(env, "logistic", 100, kind="exponential")
    env["AGP"].train_(model, 2)
    dv, ds = C.c_double(np.nan), (C.c_double * 3)(np.nan, np.nan, np.nan)
    assert capi.lib().agp_svgp_hypergrad(model._h, 0, C.byref(dv), ds, None) == 5  # AGP_ERR_UNSUPPORTED
    assert np.isnan(dv.value) and all(np.isnan(list(ds)))  # nothing written
    with pytest.raises(capi.AGPError) as e:
        model.hypergrad(0)
    assert e.value.status == 5 and capi.ERR_NAMES[5] == "AGP_ERR_UNSUPPORTED"


# ---- d. prior means -----------------------------------------------------------------------------------------------------------
def _vector_mean(N):
    return 0.6 * np.cos(np.arange(N) * 0.37) - 0.2


@pytest.mark.parametrize("likname,mean", [("logistic", 0.4), ("logisticsoftmax", 0.4), ("heteroscedastic", 0.4),
                                          ("logistic", "vector"), ("poisson", "vector")])
def test_vgp_prior_mean(env, likname, mean):
    N = 140
    mean = _vector_mean(N) if mean == "vector" else mean
    X, yt, model, ref = _case(env, likname, N, mean=mean)
    _run(env, model, ref, yt, (1, 2, 5))
    if not np.isscalar(mean):
        _hypergrad_vs_autograd(env, model, "sqexponential", 2.0, X, mean)


# ---- e. hyper-parameter trajectories ------------------------------------------------------------------------------------------
def _trajectory(env, likname, N, kind="sqexponential", scale=2.0, ktol=1e-9):
    """8 iterations with ADAM(0.01) (hyper steps after iterations 4..7) against the restatement's train loop: every latent's kernel
    parameters to 1e-9, the ELBO trace to 1e-8, the final state to 1e-7 (as test_vgp_hyper_trajectory)"""
    from oracle import agp_ref as R

    AGP = env["AGP"]
    X, yt, model, ref = _case(env, likname, N, optimiser=True, kind=kind, scale=scale)
    elbos, elbos_r = [], []
    AGP.train_(model, 8, callback=lambda m, s, i: elbos.append(AGP.objective(m)))
    ref.train(yt, 8, opt=R.Adam(0.01), callback=lambda r: elbos_r.append(r.elbo(yt)))
    assert model.n_latent == ref.nl
    for k in range(ref.nl):
        km, kr = model.kernels[k], ref.kernels[k]
        assert kr.sigma2 != 1.5  # the kernel did move
        assert km.variance == pytest.approx(kr.sigma2, rel=ktol), k
        sm = km.transform.v if np.ndim(kr.scale) else km.transform.s
        assert np.allclose(sm, kr.scale, rtol=ktol, atol=0), (k, sm, kr.scale)
        assert not np.allclose(kr.scale, scale, rtol=1e-6, atol=0)
    if ref.nl > 1:  # each latent moved with its own gradient
        assert len({ref.kernels[k].sigma2 for k in range(ref.nl)}) == ref.nl
    assert np.allclose(elbos, elbos_r, rtol=1e-8, atol=1e-8), (elbos, elbos_r)
    ref.refresh_K()
    _check_state(env, model, ref, yt, tol=1e-7)


# (lsm: latent 1's variance gradient is a sum of terms of size ~60-90 that cancels to 0.3 ... 0.002 over the four hyper steps, and
#  its ADAM second moment stays at sqrt(v) ~ 0.3.  The gradients agree to ~eps cond(K) = 1.4e-10 of those terms (cond ~ 1.3e6), so
#  four ADAM(0.01) steps move log(variance) apart by up to 4 * 0.01 * 1.4e-10 * 90 * 1.5 / 0.3 ~ 2.5e-9 (measured: 1.45e-9); the
#  kernel parameters of every latent are compared to 1e-8, and ELBO trace and state keep the bounds of the single-latent case)
@pytest.mark.parametrize("likname,N,kind,scale,ktol", [("logistic", 180, "matern52", ARD, 1e-9),
                                                       ("logisticsoftmax", 180, "sqexponential", 2.0, 1e-8),
                                                       ("logistic", 2049, "sqexponential", 2.0, 1e-9)],
                         ids=["matern52-ard", "lsm-every-latent", "se-2049-per-column"])
def test_vgp_hyper_trajectories(env, likname, N, kind, scale, ktol):
    _trajectory(env, likname, N, kind, scale, ktol)


# ---- 3. the in-stream fallback (AGP_DAG_TEST_ABORT=1: every task-graph launch is marked as having lost a dependency after it has
# finished; k_chol_safe then rebuilds A = -2 eta2 and the eta1 row, or K from Z = X, and refactors in stream) ------------------
def _retries(model):
    from agp_amd import capi

    f = capi.lib().agp_dev_dag_retries
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64()
    assert f(model._ctx, C.byref(n)) == 0
    return int(n.value)


def fallback_parity_child():
    """in the child: state and ELBO after 3 steps, one train_ call each (its status check at the end pauses the task graph)"""
    import _knobs as K_
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    env_ = dict(AGP=AGP, capi=capi, R=R)
    for N in (64, 173, 1000):
        for likname in ("logistic", "logisticsoftmax"):
            X, yt, m, ref = _case(env_, likname, N, seed=9)
            AGP.train_(m, 3)
            for _ in range(3):
                ref.step(yt)
            _check_state(env_, m, ref, yt)
            if not K_.no_task_graph():
                assert _retries(m) > 0, (N, likname)
    print("OK")


def fallback_hyper_child():
    """in the child: the SE / logistic trajectory at N = 180; the refreshes of K after the hyper steps are refactored by the
    fallback from Z = X (its kz rebuild), which the retry count after the first hyper step shows"""
    import _knobs as K_
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    env_ = dict(AGP=AGP, capi=capi, R=R)
    X, yt, model, ref = _case(env_, "logistic", 180, optimiser=True)
    elbos, elbos_r, counts = [], [], []

    def cb(m, s, i):
        elbos.append(AGP.objective(m))
        counts.append(_retries(m))

    AGP.train_(model, 8, callback=cb)
    ref.train(yt, 8, opt=R.Adam(0.01), callback=lambda r: elbos_r.append(r.elbo(yt)))
    k = model.kernels[0]
    assert k.variance == pytest.approx(ref.kernel.sigma2, rel=1e-9)
    assert float(k.transform.s) == pytest.approx(ref.kernel.scale, rel=1e-9)
    assert np.allclose(elbos, elbos_r, rtol=1e-8, atol=1e-8), (elbos, elbos_r)
    ref.refresh_K()
    _check_state(env_, model, ref, yt, tol=1e-7)
    if not K_.no_task_graph():
        assert counts[0] > 0 and counts[-1] > counts[3], counts  # the fallback also ran after the hyper steps
    print("OK")


@pytest.mark.parametrize("child", ["fallback_parity_child", "fallback_hyper_child"])
def test_vgp_in_stream_fallback(built, child):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.'); import test_gpu_vgp_edges as T; T.{child}()"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, AGP_DAG_TEST_ABORT="1"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
