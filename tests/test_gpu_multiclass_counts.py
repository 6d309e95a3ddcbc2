"""The multi-class paths on the MI355X at every class count that changes a launch (the cases and the seam each one reaches:
tests/_multiclass_cases.py; tests/test_multiclass_cases_host.py recomputes them from the constants in csrc/).

a. analytic LogisticSoftMax SVGP at K in {2, 5, 9, 10, 16, 17} against the oracle: k_lsm_fused<T, LG> at LG = 2, 8 (idle lanes),
   16 (idle and full) and the five-launch fallback; task-graph chunks 2, 5, 5+4, 5+5, 8+8, 6+6+5; k_rowstats_local at exactly 16 and
   at 16 + 1; the batched and the per-latent eta step.
b. K in {16, 17} again in a child process under AGP_CHOL_DAG=0: a full 16-problem potrf_fused_batch, and 16 + the lone seventeenth
   latent on the single-problem branch of a multi-latent handle.
c. K = 10 on the full model (VGP) and with hyper steps (per-latent kernels and inducing sets differ after the first one).
d. agp_mc_expectations point by point at K in {4, 5, 9, 16, 17, 32, 33, 64}: P = 4 .. 64 lanes per draw with and without idle
   lanes, nMC at, just above and far above one LDS tile, exact ties for the first maximum.
f. agp_log_predictive's multi-class branch at K in {2, 10, 17}.
g. MOSVGP with MO_MAXT = 16 tasks, and the refusal of 17.
(e., the Monte-Carlo trajectories at K = 10 and 17, are cases of tests/test_gpu_mcvi.py.)

Not reachable at test size: a task-graph chunk of one latent (dag_nb = 1 needs m >= 1024 with B >= 8128)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _knobs as KN
import _lpd_ref as Rf
import _mcvi_cases as CS
import _mcvi_ref as M
import _multiclass_cases as MK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, LABELS = 1, 5, 6  # include/agp_hip.h


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

    return dict(AGP=AGP, capi=capi, R=R, torch=torch)


def _kernel(AGP):
    return MK.ANALYTIC["variance"] * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(MK.ANALYTIC["scale"]))


# ---- a., b. the analytic model --------------------------------------------------------------------------------------------------------
def _analytic_run(AGP, capi, K):
    """the device's side of a case as a dict of arrays (what the child process of b. writes to its .npz)"""
    X, y, Z, idx, Xt = MK.analytic_data(K)
    B = MK.ANALYTIC["B"]
    ma = AGP.SVGP(_kernel(AGP), AGP.LogisticSoftMaxLikelihood(K), AGP.AnalyticSVI(B), Z, optimiser=False)
    elbo = []
    AGP.train_(ma, X, y, MK.ANALYTIC["steps"], idx_stream=idx, callback=lambda mdl, s, i: elbo.append(AGP.objective(mdl, s)))
    st = [ma.get_state(l) for l in range(K)]
    mf, vf = AGP.predict_f(ma, Xt, cov=True)
    pa = AGP.proba_y(ma, Xt)
    assert sorted(pa) == list(range(1, K + 1))
    return dict(mu=np.stack([s[0] for s in st]), dsig=np.stack([np.diag(s[1]) for s in st]), eta1=np.stack([s[2] for s in st]),
                eta2=np.stack([s[3] for s in st]), elbo=np.array(elbo), alpha=np.asarray(ma.get_matrix(capi.VEC_ALPHA, 0, B)),
                mean=np.stack(mf), var=np.stack(vf), proba=np.stack([pa[k] for k in range(1, K + 1)], axis=1),
                label=np.asarray(AGP.predict_y(ma, Xt)).astype(np.int64))


def _analytic_assert(K, got, what=""):
    """the bounds of tests/test_gpu_round3.py::test_many_classes_beyond_the_batched_launch_limits, per latent"""
    o = MK.analytic_oracle(K)
    lat = o["model"].latents
    e = dict(eta1=[_rel(got["eta1"][l], lat[l].eta1) for l in range(K)], eta2=[_rel(got["eta2"][l], lat[l].eta2) for l in range(K)],
             mu=[_rel(got["mu"][l], lat[l].mu) for l in range(K)], dsig=[_rel(got["dsig"][l], np.diag(lat[l].Sigma)) for l in range(K)],
             mean=[_rel(got["mean"][l], o["mean"][l]) for l in range(K)], var=[_rel(got["var"][l], o["var"][l]) for l in range(K)],
             proba=[_rel(got["proba"][:, l], o["proba"][:, l]) for l in range(K)])
    e_alpha = _rel(got["alpha"], o["model"].local_vars["alpha"])
    e_elbo = float(np.max(np.abs(got["elbo"] - o["elbo"]) / np.abs(o["elbo"])))
    print(f"K={K}{what}: worst over the latents: " + " ".join(f"{k} {max(v):.2e} (latent {int(np.argmax(v))})" for k, v in e.items())
          + f" alpha {e_alpha:.2e} ELBO {e_elbo:.2e}")
    for l in range(K):
        assert e["eta1"][l] <= 1e-9 and e["eta2"][l] <= 1e-9, (l, e["eta1"][l], e["eta2"][l])
        assert e["mu"][l] <= 1e-8 and e["dsig"][l] <= 1e-8, (l, e["mu"][l], e["dsig"][l])
        assert e["mean"][l] <= 1e-8 and e["var"][l] <= 1e-6 and e["proba"][l] <= 1e-8, (l, e["mean"][l], e["var"][l], e["proba"][l])
    assert got["elbo"].shape == (MK.ANALYTIC["steps"],) and np.allclose(got["elbo"], o["elbo"], rtol=1e-8, atol=0.0)
    assert e_alpha <= 1e-9
    assert np.array_equal(got["label"], 1 + np.argmax(got["mean"], axis=0))  # the first maximum of the device's own means


@pytest.mark.parametrize("K", list(MK.ANALYTIC_CASES))
def test_analytic_lsm_at_every_class_count(env, K):
    """m = 70, D = 3, N = 400, AnalyticSVI(150), 4 steps: every latent's eta1, eta2 <= 1e-9, mu, diag Sigma <= 1e-8, the ELBO of
    every step rtol 1e-8, alpha <= 1e-9; on 37 test points predict_f mean <= 1e-8, variance <= 1e-6, proba_y <= 1e-8, predict_y the
    first-maximum argmax of the device's means"""
    _analytic_assert(K, _analytic_run(env["AGP"], env["capi"], K))


def no_task_graph_child(path):
    """in a child process (AGP_CHOL_DAG is read once per process): the cases of b., written to path"""
    import agp_amd as AGP
    from agp_amd import capi

    assert KN.no_task_graph()
    out = {}
    for K in MK.NO_TASK_GRAPH_KS:
        out.update({f"{K}/{k}": v for k, v in _analytic_run(AGP, capi, K).items()})
    np.savez(path, **out)
    print("OK")


@pytest.mark.skipif(KN.no_task_graph(), reason="AGP_CHOL_DAG=0 is this run's setting: test_analytic_lsm_at_every_class_count took that path")
def test_analytic_lsm_without_the_task_graph(built, tmp_path):
    """K = 16 and 17 under AGP_CHOL_DAG=0: the factorisations go out as one full CholBatch of 16 (potrf_fused_batch), and as 16 + 1
    -- the seventeenth latent alone on the single-problem potrf_fused branch of a multi-latent handle.  The same bounds."""
    path = str(tmp_path / "states.npz")
    code = ("import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.'); import test_gpu_multiclass_counts as T; "
            f"T.no_task_graph_child({path!r})")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, AGP_CHOL_DAG="0"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(path)
    for K in MK.NO_TASK_GRAPH_KS:
        _analytic_assert(K, {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{K}/")}, what=" (AGP_CHOL_DAG=0)")


# ---- c. K = 10 on the full model and with hyper steps ---------------------------------------------------------------------------------
def test_vgp_ten_classes(env):
    """VGP, AnalyticVI, LogisticSoftMax(10), N = 65 (two tiles): state, local variables and ELBO after 1, 2 and 3 steps and the
    predictions, at the bounds of tests/test_gpu_vgp_edges.py (1e-8; variances by _var_tol)"""
    from _vgp_ref import VGPRef
    from test_gpu_vgp import _check_state
    from test_gpu_vgp_edges import _check_predictions

    AGP, R, c = env["AGP"], env["R"], MK.VGP10
    X, y = MK.vgp10_data()
    k = c["variance"] * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(c["scale"]))
    model = AGP.VGP(X, y, k, AGP.LogisticSoftMaxLikelihood(c["K"]), AGP.AnalyticVI(), optimiser=False)
    lik = R.LogisticSoftMaxLikelihood(c["K"])
    ref = VGPRef(R.Kernel("sqexponential", c["scale"], c["variance"]), lik, X)
    yt = R.treat_labels(y, lik)
    assert model.n_latent == c["K"] and np.all(np.sum(yt, axis=0) > 0)
    for it in range(c["steps"]):
        AGP.train_(model, 1, state=None if it == 0 else True)
        ref.step(yt)
        _check_state(env, model, ref, yt)
    _check_predictions(env, model, ref, np.random.default_rng(65).random((37, c["D"])))


def test_svgp_ten_classes_with_hyper_steps(env):
    """optimiser = ADAM(0.05), Zoptimiser = ADAM(0.01) on the K = 10 case, six iterations (three would take no hyper step: the loop's
    first is after the fourth iteration): after the two hyper steps every latent has a kernel and an inducing set of its own, which
    a mixed-up latent index cannot survive.  The bounds of the LogisticSoftMax case of tests/test_gpu_parity.py::
    test_training_with_hyper_steps_matches_oracle"""
    AGP, c = env["AGP"], MK.HYPER10
    X, y, Z, idx = MK.hyper10_data()
    ma = AGP.SVGP(_kernel(AGP), AGP.LogisticSoftMaxLikelihood(c["K"]), AGP.AnalyticSVI(MK.ANALYTIC["B"]), Z,
                  optimiser=AGP.ADAM(c["k_eta"]), Zoptimiser=AGP.ADAM(c["z_eta"]))
    AGP.train_(ma, X, y, c["steps"], idx_stream=idx)
    mr = MK.hyper10_oracle()
    D = MK.ANALYTIC["D"]
    worst = dict(variance=0.0, scale=0.0, Z=0.0, eta2=0.0, mu=0.0)
    for k in range(c["K"]):
        kr = mr.latents[k].kernel
        mu, Sig, e1, e2 = ma.get_state(k)
        e = dict(variance=abs(ma.kernels[k].variance - kr.sigma2) / kr.sigma2, scale=_rel(ma.kernels[k].scales(D), np.broadcast_to(kr.scale, (D,))),
                 Z=_rel(ma.Zs[k], mr.latents[k].Z), eta2=_rel(e2, mr.latents[k].eta2), mu=_rel(mu, mr.latents[k].mu))
        worst = {n: max(worst[n], v) for n, v in e.items()}
        assert e["variance"] <= 1e-8 and e["scale"] < 1e-8 and e["Z"] < 1e-8, (k, e)
        assert abs(ma.kernels[k].variance - MK.ANALYTIC["variance"]) > 1e-3  # the hypers really moved
        assert e["eta2"] < 1e-7 and e["mu"] < 1e-7, (k, e)
    print("K=10 with hyper steps: worst over the latents: " + " ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    assert len({round(float(ma.kernels[k].variance), 9) for k in range(c["K"])}) == c["K"]  # ... each its own way


# ---- d. the Monte-Carlo expectation kernel ---------------------------------------------------------------------------------------------
def _mc_lik(AGP, link, K):
    return AGP.SoftMaxLikelihood(K) if link == "softmax" else AGP.LogisticSoftMaxLikelihood(K)


@pytest.mark.parametrize("link", M.LINKS)
@pytest.mark.parametrize("K", list(MK.MC_POINT_CASES))
def test_mc_expectations_at_every_lane_layout(env, link, K):
    """41 points (ten workgroups of four waves and one with a single wave), nMC in {1, TS, TS + 1, 1000} with TS = 2048 // K draws
    per LDS tile; the points of _mcvi_cases.point_inputs and three engineered ones at var = 0: a K-way tie scored for class 0 (the
    first maximum) and for class K - 1, a two-way tie of the last two classes.  Every ell, g, h finite and within 1e-12 of the mean
    absolute per-draw term of the restatement on the bit-identical table (the bound of tests/test_gpu_mcvi.py; the float64
    restatement itself is within 3e-14 of a long-double evaluation for K up to 64, nMC up to 1000, and a missing or doubled butterfly
    stage is an error of order 1); two calls agree bitwise"""
    AGP = env["AGP"]
    c, mu, var = MK.mc_point_inputs(K)
    lik = _mc_lik(AGP, link, K)
    tiny = np.finfo(np.float64).tiny
    assert MK.mc_nmc(K)[1] == 2048 // K
    for nMC in MK.mc_nmc(K):
        eps = M.normals(CS.SEED, 5, M.STREAM_GRAD, nMC, K)
        ell, g, h = AGP.mc_expectations(lik, c, mu, var, nMC, CS.SEED, 5, M.STREAM_GRAD)
        er, gr, hr, (ea, ga, ha) = M.expectations(link, c, mu, var, eps)
        per = [np.abs(a - b) / np.maximum(s, tiny) for a, b, s in ((ell, er, ea), (g, gr, ga), (h, hr, ha))]
        errs = [float(np.max(p)) for p in per]
        where = [tuple(int(i) for i in np.unravel_index(np.argmax(p), p.shape)) for p in per]
        print(f"{link} K={K} nMC={nMC}: worst errors relative to mean |term|: ell {errs[0]:.2e} at point {where[0]} "
              f"g {errs[1]:.2e} at (latent, point) {where[1]} h {errs[2]:.2e} at {where[2]}")
        assert ell.shape == (MK.MC_POINTS,) and g.shape == h.shape == (K, MK.MC_POINTS)
        assert np.all(np.isfinite(ell)) and np.all(np.isfinite(g)) and np.all(np.isfinite(h))
        assert max(errs) < 1e-12
        again = AGP.mc_expectations(lik, c, mu, var, nMC, CS.SEED, 5, M.STREAM_GRAD)
        assert all(np.array_equal(a, b) for a, b in zip((ell, g, h), again))


def test_mc_expectations_refuse_one_and_sixty_five_classes(env):
    """K = 65 (beyond MC_KMAX) and K = 1 return AGP_ERR_UNSUPPORTED and write nothing"""
    capi, torch = env["capi"], env["torch"]
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    vp = lambda t: C.c_void_p(t.data_ptr())
    n = MK.MC_POINTS
    try:
        for kind in (capi.LIK_SOFTMAX, capi.LIK_LOGISTICSOFTMAX):
            for K in (65, 1):
                y = torch.zeros(n, dtype=torch.int32, device="cuda")
                mu = torch.zeros(K, n, dtype=torch.float64, device="cuda")
                var = torch.ones(K, n, dtype=torch.float64, device="cuda")
                ell = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                g, h = (torch.full((K, n), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
                lik = capi.LikDesc(kind, K, 0.0, 0.0)
                st = L.agp_mc_expectations(ctx, C.byref(lik), vp(y), vp(mu), vp(var), n, K, 10, CS.SEED, 5, M.STREAM_GRAD, vp(ell), vp(g), vp(h))
                torch.cuda.synchronize()
                assert st == UNSUPPORTED and capi.ERR_NAMES[st] == "AGP_ERR_UNSUPPORTED", (kind, K, st)
                assert "agp_mc_expectations" in L.agp_last_error(ctx).decode()
                assert all(bool(torch.isnan(t).all()) for t in (ell, g, h)), (kind, K)
    finally:
        L.agp_ctx_destroy(ctx)


# ---- f. the log predictive density, multi-class branch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Rf.MULTI)
@pytest.mark.parametrize("K", MK.LPD_KS)
def test_log_predictive_multiclass_counts(env, name, K):
    """64 points, means in +-30 with one class at +-800: within 1e-12 max(1, |ref|) of _lpd_ref.lpd_np; a class index of K is
    reported at its first position"""
    AGP, capi = env["AGP"], env["capi"]
    c, mu, var = MK.lpd_inputs(K)
    lik = AGP.SoftMaxLikelihood(K) if name == "softmax" else AGP.LogisticSoftMaxLikelihood(K)
    ref = Rf.lpd_np((name, K), c, mu, var)
    got = AGP.log_predictive_moments(lik, c, mu, var)
    per = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{name} K={K}: worst |device - restatement| / max(1, |ref|) = {float(np.max(per)):.2e} at point {int(np.argmax(per))}")
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert float(np.max(per)) <= 1e-12
    bad = c.copy()
    bad[[13, 40]] = K
    with pytest.raises(capi.AGPError) as e:
        AGP.log_predictive_moments(lik, bad, mu, var)
    assert e.value.status == LABELS and "point 13 " in str(e.value), str(e.value)
    assert np.array_equal(AGP.log_predictive_moments(lik, c, mu, var), got)


# ---- g. MOSVGP at the task limit ---------------------------------------------------------------------------------------------------------
def test_mosvgp_sixteen_tasks_and_the_refusal_of_seventeen(env):
    """16 tasks (Gaussian, Logistic, StudentT, Laplace cycled) on Q = 5 latents, m = 24, N = 300, AnalyticSVI(100), 3 steps, A fixed:
    k_mo_local's unrolled arrays are full.  eta1, eta2 <= 1e-9, mu <= 1e-8, the mixed means <= 1e-8 and variances <= 1e-7 of every
    task, the ELBO of every step (the bounds of tests/test_gpu_parity.py::test_multioutput_svgp_matches_oracle).  Between the second
    and the third step agp_svgp_set_multioutput with 17 tasks returns AGP_ERR_INVALID and changes nothing."""
    AGP, capi, c = env["AGP"], env["capi"], MK.MO16
    X, ys, kinds, A, Zs, idx, Xt = MK.mo16_data()
    mk = {"gaussian": lambda: AGP.GaussianLikelihood(0.05), "logistic": AGP.LogisticLikelihood,
          "studentt": lambda: AGP.StudentTLikelihood(3.0), "laplace": lambda: AGP.LaplaceLikelihood(0.3)}
    ma = AGP.MOSVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(c["scale"]), [mk[k]() for k in kinds], AGP.AnalyticSVI(c["B"]), Zs,
                    A=A.copy(), Aoptimiser=False)
    elbo = []
    cb = lambda mdl, s, i: elbo.append(AGP.objective(mdl, s))
    AGP.train_(ma, X, ys, 2, idx_stream=idx[:2], callback=cb)
    liks17 = (capi.LikDesc * 17)(*[ma.likelihood.likelihoods[t % 16].lik_desc() for t in range(17)])
    A17 = np.ascontiguousarray(np.vstack([A, A[:1]]))
    st = capi.lib().agp_svgp_set_multioutput(ma._h, 17, liks17, A17.ctypes.data_as(C.POINTER(C.c_double)), 0.0, 0.9, 0.999, 1e-8)
    assert st == INVALID
    assert capi.lib().agp_svgp_check_status(ma._h) == 0
    AGP.train_(ma, X, ys, 1, idx_stream=idx[2:3], callback=cb, state=True)
    o = MK.mo16_oracle()
    mr = o["model"]
    assert np.array_equal(ma.get_A(), A)
    e = dict(eta1=[], eta2=[], mu=[])
    for q in range(c["Q"]):
        mu, Sig, e1, e2 = ma.get_state(q)
        e["eta1"].append(_rel(e1, mr.latents[q].eta1))
        e["eta2"].append(_rel(e2, mr.latents[q].eta2))
        e["mu"].append(_rel(mu, mr.latents[q].mu))
    mf, vf = AGP.predict_f(ma, Xt, cov=True)
    e["mean"] = [_rel(mf[t], o["mean"][t]) for t in range(c["T"])]
    e["var"] = [_rel(vf[t], o["var"][t]) for t in range(c["T"])]
    print("MOSVGP 16 tasks: worst " + " ".join(f"{k} {max(v):.2e} (at {int(np.argmax(v))})" for k, v in e.items())
          + f" ELBO {float(np.max(np.abs(np.array(elbo) - o['elbo']) / np.abs(o['elbo']))):.2e}")
    assert len(mf) == c["T"] and len(elbo) == c["steps"]
    assert max(e["eta1"]) < 1e-9 and max(e["eta2"]) < 1e-9 and max(e["mu"]) < 1e-8
    assert max(e["mean"]) < 1e-8 and max(e["var"]) < 1e-7
    assert np.allclose(elbo, o["elbo"], rtol=1e-8, atol=1e-7), (elbo, o["elbo"])
