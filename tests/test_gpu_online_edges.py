"""GPU: the streaming model (OnlineSVGP: set_online_prior, online_refresh, online_snapshot, extra_kl, adopt_local,
agp_svgp_online_first_step and the online branch of hypergrad() in csrc/agp_capi.hip) where the old and the new inducing set differ
in their number of 64-tiles, against R.OnlineSVGP of the oracle on identical batches.

Every matrix of the streaming prior is `map x mp` or `map x map` (map = rup64(ma) old, mp = rup64(m) new inducing points, padded).
tests/test_gpu_online.py and tests/test_gpu_abi_layout.py only ever reach map == mp == 64 with Z_a inside Z.  The inputs here
(tests/_online_cases.py; their properties are proved on the CPU by tests/test_online_cases_host.py) reach
(map, mp) = (64, 64), (64, 128), (128, 128), (128, 192), (192, 128), (128, 64) with B on and off the tile grid, above and below m,
old sets that are not subsets of the new ones, three kernel / dimension combinations, fp32, and latents with different counts on
both sides of a tile edge.  Bounds: those of tests/test_gpu_online.py, test_hypergrad_matches_oracle and test_fp32_mode
(tests/test_gpu_parity.py); every test prints its worst relative errors.
"""
import ctypes as C

import numpy as np
import pytest

import _online_cases as OC
from _liks import agp_lik, oracle_lik

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5
SENTINEL = -7.25


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available()
    import agp_amd as AGP
    from agp_amd import capi
    from oracle import agp_ref as R

    return dict(AGP=AGP, R=R, capi=capi, torch=torch)


class Worst(dict):
    """largest value seen per name; `hit` returns it for the assertion"""

    def hit(self, name, v):
        self[name] = max(self.get(name, 0.0), float(v))
        return v

    def show(self, title):
        print(f"{title}: " + "  ".join(f"{k} {v:.1e}" for k, v in self.items()))


def _pair(env, c, sets=None, T=np.float64, k_opt=None, z_opt=None, jitter=1e-4):
    """(device model, oracle) of a case; sets: per-latent prescribed inducing sets (Scripted rule), None: the real OIPS"""
    AGP, R = env["AGP"], env["R"]
    la, lr = agp_lik(AGP, c["lik"]), oracle_lik(R, c["lik"])
    if c["lik"] == "logisticsoftmax":  # every batch must see the same mapping
        lr.class_mapping = la.class_mapping = [1, 2, 3]
        la.ind_mapping = {v: i + 1 for i, v in enumerate([1, 2, 3])}
    za = AGP.OIPS(OC.RHO) if sets is None else OC.Scripted(sets)
    zr = R.OIPS(OC.RHO) if sets is None else OC.Scripted(sets)
    ma = AGP.OnlineSVGP(OC.device_kernel(AGP, c), la, AGP.AnalyticVI(), za, optimiser=AGP.ADAM(k_opt) if k_opt else False,
                        Zoptimiser=AGP.ADAM(z_opt) if z_opt else False, T=T)
    mr = R.OnlineSVGP(OC.oracle_kernel(R, c), lr, zr, jitter=jitter, k_opt=R.Adam(k_opt) if k_opt else None,
                      z_opt=R.Adam(z_opt) if z_opt else None)
    return ma, mr


def _scripted(env, monkeypatch):
    import importlib

    monkeypatch.setattr(importlib.import_module("agp_amd.online"), "_oips_update", OC.device_rule)


def _batch(env, ma, mr, X, y, iters):
    """one arriving batch on both models; returns the objective (incl. extraKL) after every iteration: device, oracle"""
    AGP, R = env["AGP"], env["R"]
    ea, er = [], []
    AGP.train_online(ma, X, y, iterations=iters, callback=lambda m, cur, i: ea.append(AGP.online_objective(m)))
    yt = R.treat_labels(y, mr.likelihood)
    mr.train(X, y, iters, callback=lambda m, it, xx, yy: er.append(m.elbo(yt)))
    return ea, er, yt


def _state_matches(ma, mr, ea, er, w, where):
    """the comparisons and bounds of test_online_svgp_stream_matches_oracle"""
    assert [len(z) for z in ma.Zs] == [len(g["Z"]) for g in mr.latents], where
    for l, g in enumerate(mr.latents):
        assert w.hit("Z", _rel(ma.Zs[l], g["Z"])) < 1e-14, where
        mu, Sig, e1, e2 = ma.get_state(l)
        assert w.hit("eta1", _rel(e1, g["eta1"])) < 1e-8, (where, l)
        assert w.hit("eta2", _rel(e2, g["eta2"])) < 1e-8, (where, l)
        assert w.hit("mu", _rel(mu, g["mu"])) < 1e-7 and w.hit("Sigma", _rel(Sig, g["Sigma"])) < 1e-7, (where, l)
    w.hit("objective", max(abs(a - r) / max(abs(r), 1.0) for a, r in zip(ea, er)))
    assert len(ea) == len(er) and np.allclose(ea, er, rtol=1e-7, atol=1e-6), (where, ea, er)


def _predictions_match(env, ma, mr, Xt, w):
    """the comparisons and bounds at the end of test_online_svgp_stream_matches_oracle (70 points)"""
    AGP = env["AGP"]
    mfa, mfr = AGP.online_predict_f(ma, Xt, cov=True), mr.predict_f(Xt, cov=True)
    if ma.n_latent == 1:
        assert w.hit("mean_f", _rel(mfa[0], mfr[0][0])) < 1e-7 and w.hit("var_f", _rel(mfa[1], mfr[1][0])) < 1e-6
        assert w.hit("proba_y", _rel(AGP.online_proba_y(ma, Xt)[0], mr.proba_y(Xt)[0])) < 1e-7
    else:
        for l in range(ma.n_latent):
            assert w.hit("mean_f", _rel(mfa[0][l], mfr[0][l])) < 1e-7 and w.hit("var_f", _rel(mfa[1][l], mfr[1][l])) < 1e-6
        assert np.array_equal(AGP.online_predict_y(ma, Xt), mr.predict_y(Xt))


def _stream_matches(env, c, sets=None):
    ma, mr = _pair(env, c, sets)
    w = Worst()
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        ea, er, _ = _batch(env, ma, mr, X, y, c["iters"])
        assert len(ma.Zs[0]) == c["m_seq"][b], b
        _state_matches(ma, mr, ea, er, w, b)
    _predictions_match(env, ma, mr, c["Xt"], w)
    w.show(f"{c['name']} (ma, m, map, mp, B, D) {OC.combos(c)}")


# ---- 1. growth across tiles under the real OIPS rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,likname", [(1, "logistic"), (2, "logistic"), (3, "logistic"), (2, "gaussian"), (2, "logisticsoftmax")])
def test_online_growth_across_tiles(env, D, likname):
    """m = 40, 63, 64, 65, 65, 128, 130 with B = 60, 64, 65, 50, 37, 130, 129: (map, mp) = (64, 64), (64, 128), (128, 128), (128, 192);
    batches smaller than m, off the tile grid, and one that adds no point"""
    _stream_matches(env, OC.growth_case(D, likname))


# ---- 2. the old set is not inside the new one; ma above and below m ----------------------------------------------------------------
@pytest.mark.parametrize("seq", ["A", "B"])
@pytest.mark.parametrize("likname", ["logistic", "logisticsoftmax"])
def test_online_scripted_sets(env, monkeypatch, seq, likname):
    """A: m = 63, 65, 130, 70, 60, i.e. (map, mp) = (64, 128), (128, 192), (192, 128), (128, 64); B: 64, 64, 128, 129.  Matern52 with
    ARD; every set drops 3 points of the previous one and moves 5, so K~_a and the terms it multiplies are not zero"""
    _scripted(env, monkeypatch)
    c = OC.scripted_case(seq, likname)
    _stream_matches(env, c, [c["sets"]] * oracle_lik(env["R"], likname).n_latent)


# ---- 3. the streaming hyper-gradient itself --------------------------------------------------------------------------------------
@pytest.mark.parametrize("likname,D,kind", [("logistic", 2, "matern52"), ("gaussian", 9, "sqexponential")])
def test_online_hypergrad_matches_oracle(env, monkeypatch, likname, D, kind):
    """hypergrad() after the steps of every hand-over of sequence A, not applied: k_online_gkappa, the four k_gemm_tn products and the
    backward passes through K_ab and K_a at map != mp (at 130 -> 70 the pass through K_a has more tiles, 3 x 3, than any other pass of
    the handle: mp / 64 = 2 by max(B, m) / 64 = 3).  D = 9 is off the 8-grid of the MFMA kernel-matrix path.  Bound: 1e-8, as
    test_hypergrad_matches_oracle"""
    _scripted(env, monkeypatch)
    c = OC.scripted_case("A", likname, D, kind)
    ma, mr = _pair(env, c, [c["sets"]])
    w = Worst()
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        _, _, yt = _batch(env, ma, mr, X, y, c["iters"])
        for l in range(ma.n_latent):
            g = mr.hyper_gradient(X, yt, l)
            dv, ds, dz = ma._cur.hypergrad(l)
            w.hit("dvariance", abs(dv - g["dvariance"]) / max(1.0, abs(g["dvariance"])))
            w.hit("dscale", _rel(ds, g["dscale"]))
            w.hit("dZ", _rel(dz, g["dZ"]))
            assert abs(dv - g["dvariance"]) < 1e-8 * max(1.0, abs(g["dvariance"])), (b, dv, g["dvariance"])
            assert _rel(ds, g["dscale"]) < 1e-8, (b, ds, g["dscale"])
            assert _rel(dz, g["dZ"]) < 1e-8, b
    w.show(f"{c['name']} hyper-gradient (ma, m, map, mp, B, D) {OC.combos(c)}")


# ---- 4. hyper steps along the stream ---------------------------------------------------------------------------------------------
def test_online_scripted_hyper_steps(env, monkeypatch):
    """sequence A with ADAM(0.01) on the kernel and ADAM(0.001) on Z: the bounds of test_online_hyper_steps_match_oracle"""
    _scripted(env, monkeypatch)
    c = OC.scripted_case("A", "logistic")
    ma, mr = _pair(env, c, [c["sets"]], k_opt=0.01, z_opt=0.001)
    w = Worst()
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        _batch(env, ma, mr, X, y, c["iters"])
        g, k = mr.latents[0], ma._cur.kernels[0]
        assert w.hit("variance", abs(k.variance / g["kernel"].sigma2 - 1.0)) < 1e-7, b
        assert w.hit("scales", _rel(np.asarray(k.transform.v, dtype=float), g["kernel"].scale)) < 1e-7, b
        assert len(ma.Zs[0]) == len(g["Z"]) == c["m_seq"][b] and w.hit("Z", _rel(ma.Zs[0], g["Z"])) < 1e-7, b
        mu, Sig, e1, e2 = ma.get_state(0)
        assert w.hit("eta2", _rel(e2, g["eta2"])) < 1e-6 and w.hit("mu", _rel(mu, g["mu"])) < 1e-6, b
    w.show(f"{c['name']} with hyper steps (ma, m, map, mp, B, D) {OC.combos(c)}")


# ---- 5. more old inducing points than the gradient's scratch holds: refused, nothing else disturbed ------------------------------------
def test_online_hypergrad_refusal_leaves_the_handle_alone(env, monkeypatch):
    """130 -> 70 with B = 60 all along: Bp / 64 = 1 and mp / 64 = 2 are both below map / 64 = 3, agp_svgp_hypergrad answers
    AGP_ERR_UNSUPPORTED with the scratch message and writes no output; the CAVI steps of that hand-over match the oracle all the same,
    and a further step gives the same bits as on a handle that never asked for the gradient"""
    _scripted(env, monkeypatch)
    torch, L = env["torch"], env["capi"].lib()
    c = OC.scripted_case("A", "logistic", B=60)
    (ma, mr), (mb, _) = _pair(env, c, [c["sets"]]), _pair(env, c, [c["sets"]])
    w = Worst()
    for b in range(4):
        X, y = c["Xs"][b], c["ys"][b]
        ea, er, _ = _batch(env, ma, mr, X, y, c["iters"])
        _state_matches(ma, mr, ea, er, w, b)
        # the twin is asked for the same things in the same order, but never for the gradient
        env["AGP"].train_online(mb, X, y, iterations=c["iters"], callback=lambda m, cur, i: env["AGP"].online_objective(m))
        mb.get_state(0)
    assert (len(mr.latents[0]["Za"]), len(ma.Zs[0]), ma._cur._max_batch) == (130, 70, 60)
    cur = ma._cur
    dv, ds = C.c_double(SENTINEL), (C.c_double * cur.D)(*([SENTINEL] * cur.D))
    dZ = torch.full((cur.m, cur.D), SENTINEL, dtype=torch.float64, device="cuda")
    st = L.agp_svgp_hypergrad(cur._h, 0, C.byref(dv), ds, C.c_void_p(dZ.data_ptr()))
    msg = L.agp_last_error(cur._ctx).decode()
    assert st == UNSUPPORTED and "more old inducing points than the scratch was sized for" in msg, (st, msg)
    cur._chk(L.agp_ctx_sync(cur._ctx))
    assert dv.value == SENTINEL and all(v == SENTINEL for v in ds) and bool((dZ == SENTINEL).all())
    states = []
    for model in (ma, mb):
        h, (Xd, yd, B) = model._cur, model._data
        h._chk(L.agp_svgp_cavi_step(h._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), None, B, 1.0))
        states.append(h.get_state(0))
    print("step after the refusal against the twin, largest differences (mu, Sigma, eta1, eta2): "
          + " ".join(f"{np.max(np.abs(a - b_)):.1e}" for a, b_ in zip(*states)))
    for a, b_ in zip(*states):
        assert np.array_equal(a, b_)
    w.show(f"{c['name']} up to the refused gradient (ma, m, map, mp, B, D) {OC.combos(c)[:3]}")


# ---- 6. fp32 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["growth", "scripted-B"])
@pytest.mark.parametrize("likname", ["logistic", "logisticsoftmax"])
def test_online_fp32(env, monkeypatch, which, likname):
    """T = Float32 streaming against the fp64 oracle at jitter 1e-3: same inducing-point counts, predictive mean on 70 points within
    2e-3 (5e-3 per latent for several latents), the bounds of test_fp32_mode.  Measured on an MI355X (every run prints them):
    growth, logistic 7.8e-7; scripted B, logistic 9.6e-7; growth, logistic-softmax 6.9e-7 / 6.0e-7 / 8.1e-7 per latent; scripted B,
    logistic-softmax 9.1e-7 / 9.4e-7 / 8.0e-7 -- three orders below the bounds at cond(K) <= 11, so the bounds stay as they are."""
    if which == "growth":
        c, sets = OC.growth_case(2, likname), None
    else:
        _scripted(env, monkeypatch)
        c = OC.scripted_case("B", likname)
        sets = [c["sets"]] * oracle_lik(env["R"], likname).n_latent
    ma, mr = _pair(env, c, sets, T=np.float32, jitter=1e-3)
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        _batch(env, ma, mr, X, y, c["iters"])
        assert [len(z) for z in ma.Zs] == [len(g["Z"]) for g in mr.latents] == [c["m_seq"][b]] * ma.n_latent, b
    mf, mfr = env["AGP"].online_predict_f(ma, c["Xt"]), mr.predict_f(c["Xt"])
    errs = [_rel(mf, mfr[0])] if ma.n_latent == 1 else [_rel(mf[l], mfr[l]) for l in range(ma.n_latent)]
    print(f"{c['name']} fp32, predictive mean against the fp64 oracle: " + " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < (2e-3 if ma.n_latent == 1 else 5e-3), errs


# ---- 7. latents with different counts on both sides of a tile edge -------------------------------------------------------------------
def test_online_multilatent_counts_straddle_tiles(env, monkeypatch):
    """three latents on the growth stream: latent 0 has m = 40, 63, 64, 65, 65, 128, 130, latents 1 and 2 three points fewer (the
    last three / the first three left out), so the neutral padding of online._pad_inducing reaches across 64 and 128 while the real
    counts lie on both sides.  Kernel steps on, as in test_online_multilatent_with_different_inducing_counts, and its bounds"""
    _scripted(env, monkeypatch)
    AGP, R = env["AGP"], env["R"]
    c = OC.growth_case(2, "logisticsoftmax")
    s0 = OC.growth_sets(2)
    sets = [s0, [s[:-3] for s in s0], [s[3:] for s in s0]]
    ma, mr = _pair(env, c, sets, k_opt=0.02)
    w = Worst()
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        ea, er, _ = _batch(env, ma, mr, X, y, 6)
        w.hit("objective", max(abs(a - r) / max(abs(r), 1.0) for a, r in zip(ea, er)))
        assert np.allclose(ea, er, rtol=1e-6, atol=1e-5), (b, ea, er)
        counts = [len(g["Z"]) for g in mr.latents]
        assert counts == [c["m_seq"][b], c["m_seq"][b] - 3, c["m_seq"][b] - 3] and [len(z) for z in ma.Zs] == counts, b
        for l, g in enumerate(mr.latents):
            assert w.hit("Z", _rel(ma.Zs[l], g["Z"])) < 1e-7
            mu, Sig, e1, e2 = ma.get_state(l)
            assert w.hit("eta2", _rel(e2, g["eta2"])) < 1e-8 and w.hit("mu", _rel(mu, g["mu"])) < 1e-8, (b, l)
            assert w.hit("Sigma", _rel(Sig, g["Sigma"])) < 1e-8, (b, l)
            assert w.hit("variance", abs(ma._cur.kernels[l].variance / g["kernel"].sigma2 - 1.0)) < 1e-9, (b, l)
    pa, pr = AGP.online_predict_f(ma, c["Xt"], cov=True), mr.predict_f(c["Xt"], cov=True)
    for l in range(3):
        assert w.hit("mean_f", _rel(pa[0][l], pr[0][l])) < 1e-6 and w.hit("var_f", _rel(pa[1][l], pr[1][l])) < 1e-6
    assert np.array_equal(AGP.online_predict_y(ma, c["Xt"]), mr.predict_y(c["Xt"]))
    w.show(f"{c['name']} with counts (m, m - 3, m - 3)")
