"""MOVGP (the multi-output full variational GP: AGP_FLAG_FULL handle with the multi-output likelihood) on the MI355X against the
NumPy restatement tests/_movgp_ref.py, on the inputs of tests/_movgp_cases.py (whose boundedness tests/test_movgp_host.py checks).

Tolerances: the project's 1e-8 relative on state and ELBO (README.md, test_gpu_vgp.py::_check_state), 1e-7 after hyper steps
(test_vgp_hyper_trajectory)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _movgp_cases as MC

pytestmark = pytest.mark.gpu


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


def _pair(env, case, optimiser=False, a_opt="case"):
    """(X, treated targets, device model, restatement) of a case"""
    AGP, R = env["AGP"], env["R"]
    X, ys, yt, A, mean, ref = MC.make_ref(case, R, a_opt="case" if a_opt == "case" else (R.Adam(0.01) if a_opt else None))
    model = MC.make_model(case, AGP, X, ys, A, mean, optimiser=optimiser,
                          a_opt="case" if a_opt == "case" else (AGP.ADAM(0.01) if a_opt else False))
    return X, yt, model, ref


def _check_state(env, model, ref, yt, tol=1e-8):
    """eta1, eta2, mu, Sigma per latent, A, every task's theta, and objective"""
    AGP, capi = env["AGP"], env["capi"]
    assert AGP.n_latent(model) == ref.nl
    for q in range(ref.nl):
        mu, Sig, e1, e2 = model.get_state(q)
        assert _rel(e1, ref.eta1[q]) < tol, ("eta1", q, _rel(e1, ref.eta1[q]))
        assert _rel(e2, ref.eta2[q]) < tol, ("eta2", q, _rel(e2, ref.eta2[q]))
        assert _rel(mu, ref.mu[q]) < tol, ("mu", q, _rel(mu, ref.mu[q]))
        assert _rel(Sig, ref.Sigma[q]) < tol, ("Sigma", q, _rel(Sig, ref.Sigma[q]))
    assert _rel(model.get_A(), ref.A) < tol
    n = len(ref.X)
    for t in range(ref.n_task):
        th = model.get_matrix(capi.VEC_THETA, t, n)
        assert _rel(th, ref.lv[t]["theta"]) < tol, ("theta", t, _rel(th, ref.lv[t]["theta"]))
    ea, er = AGP.objective(model), ref.elbo(yt)
    assert abs(ea - er) < tol * max(1.0, abs(er)), (ea, er)


def _train_both(env, model, ref, yt, stops=(1, 2, 10)):
    AGP = env["AGP"]
    done = 0
    for it in stops:
        AGP.train_(model, it - done, state=None if done == 0 else True)
        for _ in range(it - done):
            ref.step(yt)
        done = it
        _check_state(env, model, ref, yt)


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_movgp_parity(env, case):
    """state, A, local variables and objective after 1, 2 and 10 iterations"""
    X, yt, model, ref = _pair(env, case)
    _train_both(env, model, ref, yt)
    mm, cc = MC.bounded(ref)
    assert mm <= MC.MAX_MU and cc <= MC.MAX_COND  # (the condition of the case table, on the trajectory just compared)
    if case["aopt"] and case["Q"] > 1:
        assert not np.array_equal(ref.A, MC.make_data(case)[2])  # A did move
    # mean_f / var_f of the last local phase: mu_q, diag Sigma_q of the posterior BEFORE the last step
    capi = env["capi"]
    assert model.get_matrix(capi.VEC_MEAN_F, case["Q"] - 1, case["N"]).shape == (case["N"],)
    assert np.all(model.get_matrix(capi.VEC_VAR_F, 0, case["N"]) > 0)


def test_movgp_mean_f_var_f_are_the_previous_posterior(env):
    case = MC.EXTRA["child-173"][0]
    capi = env["capi"]
    X, yt, model, ref = _pair(env, case)
    env["AGP"].train_(model, 3)
    for _ in range(2):
        ref.step(yt)
    for q in range(2):  # what the third step's local phase saw
        assert _rel(model.get_matrix(capi.VEC_MEAN_F, q, 173), ref.mu[q]) < 1e-8
        assert _rel(model.get_matrix(capi.VEC_VAR_F, q, 173), np.diag(ref.Sigma[q])) < 1e-8


def _fallbacks(env, model):
    n = C.c_int64()
    env["capi"].lib().agp_ctx_task_graph_fallbacks(model._ctx, C.byref(n))
    return n.value


def test_movgp_parity_large(env):
    """N = 2048, Q = 3, Logistic + Laplace, 3 iterations; no task-graph launch fell back"""
    X, yt, model, ref = _pair(env, MC.LARGE)
    env["AGP"].train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    _check_state(env, model, ref, yt)
    assert _fallbacks(env, model) == 0


def parity_child():
    """in a child process: three cases (two and three tasks, Q = 2, 3; a tile edge and 1000 points) after 3 steps"""
    import _knobs as K_
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R
    from test_gpu_vgp_edges import _retries

    env_ = dict(AGP=AGP, capi=capi, R=R)
    forced = os.environ.get("AGP_DAG_TEST_ABORT") == "1"
    for name in ("child-173", "child-200", "child-1000"):
        case = MC.EXTRA[name][0]
        X, yt, model, ref = _pair(env_, case)
        model._ensure_ctx()
        before = _retries(model)
        AGP.train_(model, 3)
        for _ in range(3):
            ref.step(yt)
        _check_state(env_, model, ref, yt)
        if forced and not K_.no_task_graph():
            assert _retries(model) > before, MC.case_id(case)  # the in-stream re-run did execute
    print("OK")


def hyper_child():
    """in a child process: the hyper trajectory (K refreshed after every hyper step, refactored by whichever driver is on)"""
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    _trajectory(dict(AGP=AGP, capi=capi, R=R), "trajectory-child")
    print("OK")


def _child(name, **extra):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.'); import test_gpu_movgp as T; T.{name}()"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **extra), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("child", ["parity_child", "hyper_child"])
def test_movgp_parity_without_task_graph(built, child):
    """the per-column driver (AGP_CHOL_DAG=0), one child process, started once"""
    _child(child, AGP_CHOL_DAG="0")


@pytest.mark.parametrize("child", ["parity_child", "hyper_child"])
def test_movgp_in_stream_fallback(built, child):
    """AGP_DAG_TEST_ABORT=1 sets the dependency latch behind every task-graph launch that ran correctly, so the plain in-stream
    re-run executes too: the same state, and the re-run count moved (parity_child)"""
    _child(child, AGP_DAG_TEST_ABORT="1")


def test_movgp_predictions(env):
    AGP, R = env["AGP"], env["R"]
    for name in ("predict-3", "predict-svm-negbin", "predict-gaussian"):
        case = MC.EXTRA[name][0]
        X, yt, model, ref = _pair(env, case)
        AGP.train_(model, 4)
        for _ in range(4):
            ref.step(yt)
        Xt = np.random.default_rng(1).random((57, 3))
        mus, vars_, covs = ref.predict_f(Xt)
        # Variances and covariances: k** - diag(K*n A Kn*) cancels the digits of A's O(cond K) entries; the VGP / SVGP parity tests
        # use this 1e-6.  Measured on these inputs: means 2.2e-11 .. 4.8e-11, variances = covariances 5.2e-8 .. 3.3e-7.
        mf = AGP.predict_f(model, Xt)
        mf2, vf = AGP.predict_f(model, Xt, cov=True)
        mc, cc = AGP.predict_f(model, Xt, cov=True, diag=False)
        pa, pr = AGP.proba_y(model, Xt), ref.proba_y(Xt)
        ya, yr = AGP.predict_y(model, Xt), ref.predict_y(Xt)
        assert len(mf) == len(vf) == len(cc) == len(pa) == len(ya) == ref.n_task
        for t in range(ref.n_task):
            assert _rel(mf[t], mus[t]) < 1e-8 and _rel(mf2[t], mus[t]) < 1e-8 and _rel(vf[t], vars_[t]) < 1e-6
            assert _rel(mc[t], mus[t]) < 1e-8 and _rel(cc[t], covs[t]) < 1e-6
            # proba_y, the likelihood half on its own: the device's outputs against the oracle's compute_proba applied to the
            # device's OWN mixed (mean_f, var_f) -- the Gauss-Hermite / regression kernels at the project's 1e-8 (measured <= 1.3e-13)
            own = R.compute_proba(ref.liks[t], (mf2[t],), (vf[t],))
            assert _rel(pa[t][0], own[0]) < 1e-8 and _rel(pa[t][1], own[1]) < 1e-8
            # ... and end to end.  A regression task's first output IS the mixed mean: 1e-8.  A Bernoulli / count task's is an
            # integral over N(mean_f, var_f) and moves with var_f: |dp| <= sup |g''| / 2 * |dvar|, and 1e-6 of max var_f = 0.14 is
            # 1.4e-7, so 1e-7.  Measured: 2.8e-10 .. 1.8e-8 where var_f differs by 1.0e-7 .. 2.5e-7; second outputs 4e-9 .. 2.8e-7.
            ptol = 1e-7 if case["tasks"][t] in ("logistic", "bsvm", "negbin") else 1e-8
            assert _rel(pa[t][0], pr[t][0]) < ptol and _rel(pa[t][1], pr[t][1]) < 1e-6
            assert np.allclose(np.asarray(ya[t], float), np.asarray(yr[t], float), rtol=1e-8, atol=1e-8)


def test_movgp_elbo_after_set_state(env):
    AGP = env["AGP"]
    case = MC.EXTRA["elbo"][0]
    X, yt, model, ref = _pair(env, case)
    AGP.train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    assert AGP.ELBO(model) == pytest.approx(ref.elbo_fresh(yt), rel=1e-8)
    lv_before = [model.get_matrix(env["capi"].VEC_THETA, t, 173) for t in range(2)]
    mu, Sig, e1, e2 = model.get_state(1)
    e2b = e2 - 0.05 * np.eye(len(X))
    model.set_state(1, e1, e2b)
    ref.eta2[1] = e2b
    ref.mu[1], ref.Sigma[1] = env["R"].natural_to_standard(e1, e2b)
    ea, er = AGP.ELBO(model), ref.elbo_fresh(yt)
    assert abs(ea - er) < 1e-8 * max(1.0, abs(er)), (ea, er)
    # the fresh evaluation leaves the training state alone: local variables, A, and the next step
    for t in range(2):
        assert np.array_equal(model.get_matrix(env["capi"].VEC_THETA, t, 173), lv_before[t])
    AGP.train_(model, 1, state=True)
    ref.step(yt)
    _check_state(env, model, ref, yt)


@pytest.mark.parametrize("name", ["hypergrad-se", "hypergrad-mixed"])
def test_movgp_hypergrad(env, name):
    """the Gaussian-KL gradient of every latent's kernel after 3 steps, with a constant prior mean
    (both sides sum products of K^-1's O(cond K) entries into an O(1) gradient: 1e-6 of the result, as for VGP; measured on
    these inputs: d variance 8.7e-11 .. 3.5e-8, d scales 3.2e-13 .. 1.9e-8)"""
    case = MC.EXTRA[name][0]
    kernels = case["kernels"]
    X, yt, model, ref = _pair(env, case)
    env["AGP"].train_(model, 3)
    for _ in range(3):
        ref.step(yt)
    for q in range(2):
        dv, ds = model.hypergrad(q)
        rv, rs = ref.hyper_grad(q)
        assert dv == pytest.approx(rv, rel=1e-6), (q, dv, rv)
        if np.ndim(kernels[q % len(kernels)][1]):
            assert np.allclose(ds, rs, rtol=1e-6, atol=1e-6 * np.max(np.abs(rs))), (q, ds, rs)
        else:
            assert float(np.sum(ds)) == pytest.approx(float(np.sum(rs)), rel=1e-6), (q, ds, rs)


def _trajectory(env, name, ktol=1e-9):
    """ADAM(0.01) hyper steps inside train! (after iterations 4..7 of 8) with the Aoptimiser on: kernel parameters of every latent, A,
    the ELBO trace, then the state at 1e-7"""
    AGP, R = env["AGP"], env["R"]
    case = MC.EXTRA[name][0]
    kernels = case["kernels"]
    X, yt, model, ref = _pair(env, case, optimiser=True)
    assert model.k_opt.eta == 0.01
    elbos, elbos_r = [], []
    AGP.train_(model, 8, callback=lambda m, s, i: elbos.append(AGP.objective(m)))
    ref.train(yt, 8, opt=R.Adam(0.01), callback=lambda r: elbos_r.append(r.elbo(yt)))
    for q in range(2):
        k, kr = model.kernels[q], ref.kernels[q]
        kind, s0, v0 = kernels[q % len(kernels)]
        assert kr.sigma2 != v0 and not np.array_equal(kr.scale, s0)  # the kernel did move
        assert k.variance == pytest.approx(kr.sigma2, rel=ktol)
        got = np.asarray(k.transform.v) if np.ndim(s0) else float(k.transform.s)
        assert np.allclose(got, kr.scale, rtol=ktol, atol=0), (q, got, kr.scale)
    assert not np.array_equal(ref.A, MC.make_data(case)[2])
    assert np.allclose(elbos, elbos_r, rtol=1e-8, atol=1e-8), (elbos, elbos_r)
    ref.refresh_K()
    _check_state(env, model, ref, yt, tol=1e-7)


@pytest.mark.parametrize("name", ["trajectory-se", "trajectory-mixed"])
def test_movgp_hyper_trajectory(env, name):
    _trajectory(env, name)


def test_movgp_prior_mean_with_hyper_step_is_refused(env):
    AGP = env["AGP"]
    case = MC.EXTRA["hypergrad-se"][0]
    X, yt, model, ref = _pair(env, case, optimiser=True)
    with pytest.raises(NotImplementedError, match="a non-zero prior mean together with hyper-parameter optimisation is not wired"):
        AGP.train_(model, 8)


def test_movgp_save_load_round_trip(env, tmp_path):
    """identical predictions; both copies train on identically.  The device state of the Aoptimiser and the tasks' local variables
    (which only update_A! reads before they are overwritten) restart on load, as documented for MOSVGP: the continued runs are
    compared with the Aoptimiser off, and with it on the mixing weights travel."""
    AGP = env["AGP"]
    case = MC.EXTRA["save-load"][0]
    X, yt, model, ref = _pair(env, case, optimiser=True)
    AGP.train_(model, 5)
    f = str(tmp_path / "movgp.npz")
    AGP.save_trained_model(f, model)
    m2 = AGP.load_trained_model(f)
    assert isinstance(m2, AGP.MOVGP) and m2.N == model.N and AGP.n_latent(m2) == 2 and m2.n_task == 3
    assert m2.A_opt is None and m2.k_opt.eta == 0.01
    Xt = np.random.default_rng(4).random((31, 3))
    a, b = AGP.predict_f(model, Xt, cov=True), AGP.predict_f(m2, Xt, cov=True)
    for t in range(3):
        assert _rel(b[0][t], a[0][t]) < 1e-10 and _rel(b[1][t], a[1][t]) < 1e-10  # (measured: identical to the last bit)
    pa, pb = AGP.proba_y(model, Xt), AGP.proba_y(m2, Xt)
    for t in range(3):
        assert _rel(pb[t][0], pa[t][0]) < 1e-10 and _rel(pb[t][1], pa[t][1]) < 1e-10
    for q in (model, m2):
        AGP.train_(q, 3, state=True)
    for l in range(2):
        for u, v in zip(model.get_state(l), m2.get_state(l)):
            assert _rel(v, u) < 1e-10
        assert m2.kernels[l].variance == pytest.approx(model.kernels[l].variance, rel=1e-12)
    # Aoptimiser on, a label and a count task: A and the optimiser's rule travel
    case = MC.EXTRA["save-load-A"][0]
    X, yt, model, ref = _pair(env, case)
    AGP.train_(model, 4)
    AGP.save_trained_model(f, model)
    m3 = AGP.load_trained_model(f)
    assert np.array_equal(m3.get_A(), model.get_A()) and m3.A_opt.eta == 0.01 and m3.k_opt is None
    # the targets come back as the caller gave them: +-1 labels, integer counts
    assert m3.y[1].dtype == model.y[1].dtype == np.int64 and all(np.array_equal(u, v) for u, v in zip(m3.y, model.y))
    a, b = AGP.predict_f(model, Xt, cov=True), AGP.predict_f(m3, Xt, cov=True)
    ya, yb = AGP.predict_y(model, Xt), AGP.predict_y(m3, Xt)
    for t in range(2):
        assert _rel(b[0][t], a[0][t]) < 1e-10 and _rel(b[1][t], a[1][t]) < 1e-10
        assert np.array_equal(np.asarray(ya[t], float), np.asarray(yb[t], float))
    AGP.train_(m3, X, MC.make_data(case)[1], 1, state=True)  # (the own-data rule holds for the reloaded targets)


def test_movgp_testset_of_the_reference(env):
    """test/models/MOVGP.jl: N = 20, d = 2, Logistic + Laplace(2), num_latent = 2, MOVGP(X, ys, k, likelihoods, AnalyticVI(), 2);
    train! 10 iterations, then predict_y and proba_y run and return one finite array of length 20 per task"""
    from test_gpu_reference_suite import generate_f

    AGP = env["AGP"]
    rng = np.random.default_rng(42)
    X, f = generate_f(rng, 20, 2, 10.0, 1.0)
    _, f2 = generate_f(rng, 20, 2, 10.0, 1.0, X)
    ys = [f > 0, f2 + rng.laplace(0.0, 2.0, 20)]
    model = AGP.MOVGP(X, ys, AGP.SqExponentialKernel() @ AGP.ScaleTransform(10.0),
                      [AGP.LogisticLikelihood(), AGP.LaplaceLikelihood(2.0)], AGP.AnalyticVI(), 2)
    AGP.train_(model, 10)
    assert model.trained and AGP.n_latent(model) == 2
    yp, pp = AGP.predict_y(model, X), AGP.proba_y(model, X)
    assert len(yp) == 2 and len(pp) == 2
    for t in range(2):
        assert np.asarray(yp[t]).shape == (20,) and np.all(np.isfinite(np.asarray(yp[t], dtype=float)))
        assert np.asarray(pp[t][0]).shape == (20,) and np.all(np.isfinite(pp[t][0])) and np.all(np.isfinite(pp[t][1]))
    assert np.allclose(np.linalg.norm(model.get_A(), axis=1), 1.0)
    assert np.isfinite(AGP.objective(model)) and np.isfinite(AGP.ELBO(model))
    # train!(model, X, y, iterations) under the own-data rule
    AGP.train_(model, X, ys, 2)
    with pytest.raises(ValueError, match="trains on the data it was built with"):
        AGP.train_(model, X + 1.0, ys, 2)


def test_movgp_refusals(env):
    from test_gpu_vgp import create_status

    AGP, capi = env["AGP"], env["capi"]
    case = MC.EXTRA["refusals"][0]
    X, yt, m, ref = _pair(env, case)
    AGP.train_(m, 2)
    L, h = capi.lib(), m._h
    n0 = C.c_int64()
    L.agp_svgp_step_counters(h, C.byref(n0), C.byref(C.c_int64()))
    assert L.agp_svgp_mo_shard(h, 4) == 5
    assert L.agp_svgp_cavi_step_multi(h, None, 0, None, 3, None, None, 173, 1.0) == 5
    assert L.agp_svgp_prefetch(h, None, 3, None, 173) == 5
    assert L.agp_svgp_step_stats(h) == 5 and L.agp_svgp_step_global(h) == 5
    assert L.agp_svgp_elbo_multi(h, None, 0, C.byref(C.c_double())) == 5
    assert L.agp_svgp_hyper_step_multi(h, None, 0) == 5
    assert L.agp_svgp_mo_mix(h) == 5 and L.agp_svgp_mo_refresh_f(h) == 5
    assert L.agp_svgp_hypergrad(h, 0, C.byref(C.c_double()), None, C.c_void_p(1)) == 5
    n1 = C.c_int64()
    L.agp_svgp_step_counters(h, C.byref(n1), C.byref(C.c_int64()))
    assert n1.value == n0.value == 2  # refused before anything was counted or enqueued
    AGP.train_(m, 1, state=True)  # nothing changed: the model still trains, and on the reference's trajectory
    for _ in range(3):
        ref.step(yt)
    _check_state(env, m, ref, yt)
    # descriptors: exact GP with a multi-output likelihood, a latent offset, a minibatch handle
    MO = capi.LikDesc(capi.LIK_MULTIOUTPUT, 2, 0.0, 0.0)
    for fields, status, msg in [(dict(lik=MO, n_latent=2, flags=capi.FLAG_FULL | capi.FLAG_EXACT), 5,
                                 "one latent and a Gaussian likelihood"),
                                (dict(lik=MO, n_latent=2, latent_offset=1), 1, "all of its latents on one handle"),
                                (dict(lik=MO, n_latent=2, max_batch=32), 1, "max_batch = m = N"),
                                (dict(lik=MO, n_latent=2, stochastic=1, rm_kappa=0.75, rm_tau=1.0), 1, "max_batch = m = N"),
                                (dict(lik=MO, n_latent=2, dtype=capi.F32), 5, "Float64 only")]:
        st, err = create_status(capi, **fields)
        assert st == status and msg in err, (fields, st, err)
    assert create_status(capi, lik=MO, n_latent=2)[0] == 0  # ... and the MOVGP descriptor itself is accepted


def test_mosvgp_exports_the_tasks_local_variables_too(env):
    """AGP_VEC_THETA / AGP_VEC_C count the tasks on every multi-output handle: the sparse model's theta against the oracle"""
    AGP, R, capi = env["AGP"], env["R"], env["capi"]
    case = MC.EXTRA["child-173"][0]
    X, ys, yt, A, mean, ref = MC.make_ref(case, R)
    Zs = [X[:24].copy(), X[24:48].copy()]
    ma = AGP.MOSVGP(1.5 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0)), [MC.TASKS[t][1](AGP) for t in case["tasks"]],
                    AGP.AnalyticVI(), Zs, A=A.copy(), Aoptimiser=AGP.ADAM(0.01))
    mr = R.MOSVGP(R.Kernel("sqexponential", 2.0, 1.5), ref.liks, Zs, A.copy(), A_opt=R.Adam(0.01))
    AGP.train_(ma, X, ys, 3)
    mr.train(X, yt, 3)
    for t in range(2):
        assert _rel(ma.get_matrix(capi.VEC_THETA, t, 173), mr.local_vars[t]["theta"]) < 1e-8
