"""GPU: pathwise posterior sampling (include/agp_hip.h "PATHWISE SAMPLING", csrc/agp_pathwise.h, pathwise.py) against the NumPy
restatement tests/_pathwise_ref.py.  The random tables (Omega, phases, W, E) are compared bit for bit; V and the evaluated paths
against the restatement fed with the handle's own exported state, to the project's parity bound of 1e-8 relative in max norm.
Inputs as in tests/_nvi_cases.py: X ~ N(0, 1) in three dimensions against a length scale of 1 / 3, so K + jitt I is well conditioned.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _pathwise_ref as P
from _pitched import Pitched, layouts

pytestmark = pytest.mark.gpu

PARITY = 1e-8
KIND, SCALE, SIGMA2 = "sqexponential", 3.0, 1.5
KINDS = dict(zip(P.KINDS, ("SqExponentialKernel", "Matern52Kernel", "Matern32Kernel", "ExponentialKernel")))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    yield dict(AGP=AGP, capi=capi, L=L, ctx=ctx, torch=torch)
    L.agp_ctx_destroy(ctx)


def _kernel(AGP, kind=KIND, scale=SCALE, sigma2=SIGMA2):
    tr = AGP.ScaleTransform(scale) if np.isscalar(scale) else AGP.ARDTransform(list(scale))
    return sigma2 * (getattr(AGP, KINDS[kind])() @ tr)


def _data(N, seed=3, D=3):
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    f = np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] ** 2 - 0.7
    return rng, X, f


@functools.lru_cache(maxsize=None)
def _svgp(m):
    """SVGP, Logistic, AnalyticSVI(50) after 5 steps on 300 points, m inducing points"""
    import agp_amd as AGP

    rng, X, f = _data(300)
    y = np.sign(f + 0.3 * rng.standard_normal(len(X)))
    Z = rng.standard_normal((m, 3))
    model = AGP.SVGP(_kernel(AGP), AGP.LogisticLikelihood(), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    return model, Z, (X, y)


XT = np.random.default_rng(99).standard_normal((200, 3))


def _check_latent(paths, l, ref, F, errs):
    """tables bit for bit, V and the paths of latent l to the parity bound; ref is the restated draw with V formed"""
    tb = paths.tables(l)
    for name, want in (("omega", ref.omega), ("phase", ref.phase), ("W", ref.W), ("E", ref.E)):
        assert np.array_equal(tb[name], want), name
    errs.append((_rel(tb["V"], ref.V), _rel(F, ref(XT[:F.shape[1]]))))
    assert errs[-1][0] < PARITY and errs[-1][1] < PARITY, errs[-1]


# ---- the spectral draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
def test_spectral_draw_is_the_restatement_bit_for_bit(env, kind):
    L, ctx, torch, AGP = env["L"], env["ctx"], env["torch"], env["AGP"]
    n = 0
    for D in (1, 3, 33):
        for scale in (2.0, tuple(0.5 + 0.1 * d for d in range(D))):  # ScaleTransform and ARD: the draw does not read the scales
            kd, keep = _kernel(AGP, kind, scale).desc(D)
            for nf in (1, 63, 64, 65, 200):
                for latent in (0, 3):
                    for t in (0, 2 ** 32 - 1):
                        om = torch.full((nf, D), float("nan"), dtype=torch.float64, device="cuda")
                        ph = torch.full((nf,), float("nan"), dtype=torch.float64, device="cuda")
                        assert L.agp_pathwise_features(ctx, C.byref(kd), D, nf, C.c_uint64(2 ** 63 + 12345), t, latent,
                                                       C.c_void_p(om.data_ptr()), C.c_void_p(ph.data_ptr())) == 0
                        ro, rp = P.features(kind, D, nf, 2 ** 63 + 12345, t, latent)
                        assert np.array_equal(om.cpu().numpy(), ro) and np.array_equal(ph.cpu().numpy(), rp), (D, nf, latent, t)
                        n += 1
    assert n == 3 * 2 * 5 * 2 * 2


def test_host_wrapper_of_the_spectral_draw(env):
    AGP = env["AGP"]
    om, ph = AGP.pathwise_features(_kernel(AGP, "matern52", (1.0, 2.0)), 2, 70, seed=9, t=4, latent=1)
    ro, rp = P.features("matern52", 2, 70, 9, 4, 1)
    assert np.array_equal(om, ro) and np.array_equal(ph, rp)


# ---- tables, V and the paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_svgp_tables_V_and_paths(env, m):
    AGP = env["AGP"]
    model, Z, _ = _svgp(m)
    mu, Sig, e1, e2 = model.get_state(0)
    errs = []
    for nf in (1, 65, 200):
        for S in (1, 63, 65):
            paths = AGP.sample_paths(model, S, n_features=nf, seed=77, t=nf + S)
            ref = P.Draw(KIND, SCALE, SIGMA2, Z, S, nf, 77, nf + S).sparse(mu, e2)
            for nt in (1, 63, 200):
                F = paths(XT[:nt])
                assert F.shape == (S, nt)
                _check_latent(paths, 0, ref, F, errs)
            paths.free()
    print(f"m = {m}: largest relative error of V {max(e[0] for e in errs):.2e}, of the paths {max(e[1] for e in errs):.2e}")


def _multi_latent(env, model, Zs, S=5, nf=65):
    AGP = env["AGP"]
    paths = AGP.sample_paths(model, S, n_features=nf, seed=5, t=1)
    F = paths(XT[:63])
    assert F.shape == (model.n_latent, S, 63)
    errs = []
    for l in range(model.n_latent):
        mu, Sig, e1, e2 = model.get_state(l)
        ref = P.Draw(KIND, SCALE, SIGMA2, Zs[l], S, nf, 5, 1, latent=l).sparse(mu, e2)
        _check_latent(paths, l, ref, F[l], errs)
    assert not np.array_equal(paths.tables(0)["W"], paths.tables(1)["W"])  # per-latent streams
    print("largest relative errors (V, paths) per latent:", errs)


def test_logisticsoftmax_draws_one_path_set_per_latent(env):
    AGP = env["AGP"]
    rng, X, f = _data(300)
    y = 1 + (f > -0.9).astype(int) + (f > 0.0).astype(int)
    Z = rng.standard_normal((65, 3))
    model = AGP.SVGP(_kernel(AGP), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    _multi_latent(env, model, model.Zs)


def test_heteroscedastic_draws_both_latents(env):
    AGP = env["AGP"]
    rng, X, f = _data(300)
    y = f + 0.2 * rng.standard_normal(len(X))
    Z = rng.standard_normal((64, 3))
    model = AGP.SVGP(_kernel(AGP), AGP.HeteroscedasticLikelihood(1.0), AGP.AnalyticSVI(50), Z, optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    _multi_latent(env, model, model.Zs)


def test_online_handle_is_an_ordinary_sparse_handle(env):
    AGP = env["AGP"]
    rng = np.random.default_rng(17)
    X = rng.random((240, 2)) * np.array([5.0, 2.0])
    y = np.sign(np.sin(2 * X[:, 0]) + 0.5 * np.cos(3 * X[:, 1]) + 0.2 * rng.standard_normal(len(X)))
    ma = AGP.OnlineSVGP(1.2 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(1.5)), AGP.LogisticLikelihood(), AGP.AnalyticVI(),
                        AGP.OIPS(0.7), optimiser=False)
    for b in range(0, len(X), 60):
        AGP.train_online(ma, X[b:b + 60], y[b:b + 60], iterations=3)
    cur = ma._cur
    mu, Sig, e1, e2 = cur.get_state(0)
    paths = AGP.sample_paths(ma, 7, n_features=65, seed=3, t=0)
    xt = rng.random((63, 2)) * np.array([5.0, 2.0])
    ref = P.Draw("sqexponential", 1.5, 1.2, cur.Zs[0], 7, 65, 3, 0).sparse(mu, e2)
    tb = paths.tables(0)
    assert np.array_equal(tb["W"], ref.W) and np.array_equal(tb["E"], ref.E)
    ev, ef = _rel(tb["V"], ref.V), _rel(paths(xt), ref(xt))
    print(f"online handle, m = {cur.m}: relative error of V {ev:.2e}, of the paths {ef:.2e}")
    assert ev < PARITY and ef < PARITY


def test_vgp_draw(env):
    AGP = env["AGP"]
    rng, X, f = _data(70)
    y = np.sign(f + 0.3 * rng.standard_normal(len(X)))
    model = AGP.VGP(X, y, _kernel(AGP, "matern52"), AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
    AGP.train_(model, 5)
    mu, Sig, e1, e2 = model.get_state(0)
    errs = []
    for S, nf in ((1, 1), (65, 200)):
        paths = AGP.sample_paths(model, S, n_features=nf, seed=21, t=S)
        ref = P.Draw("matern52", SCALE, SIGMA2, X, S, nf, 21, S).sparse(mu, e2)
        _check_latent(paths, 0, ref, paths(XT[:63]), errs)
    print("VGP, N = 70: largest relative errors (V, paths)", errs)


def test_exact_gp_draw(env):
    AGP = env["AGP"]
    rng, X, f = _data(70)
    y = f + 0.1 * rng.standard_normal(len(X))
    noise = 0.05
    model = AGP.GP(X, y, _kernel(AGP, "matern32"), noise=noise, opt_noise=False, optimiser=False)
    AGP.train_(model, 3)
    alpha, Sy = model.get_state(0)
    errs = []
    for S, nf in ((1, 1), (65, 200)):
        paths = AGP.sample_paths(model, S, n_features=nf, seed=22, t=S)
        ref = P.Draw("matern32", SCALE, SIGMA2, X, S, nf, 22, S).exact(alpha, Sy, noise)
        _check_latent(paths, 0, ref, paths(XT[:63]), errs)
    print("GP, N = 70: largest relative errors (V, paths)", errs)


# ---- a draw is a function --------------------------------------------------------------------------------------------------------
def test_paths_do_not_depend_on_where_a_point_stands(env):
    AGP, torch = env["AGP"], env["torch"]
    model, Z, _ = _svgp(64)
    paths = AGP.sample_paths(model, 3, n_features=65, seed=8, t=0)
    F = paths(XT)
    perm = np.random.default_rng(1).permutation(len(XT))
    Fp = paths(XT[perm])
    big = np.concatenate([XT, np.random.default_rng(2).standard_normal((4097 - len(XT), 3))])
    big = np.roll(big, 4000, axis=0)  # the 200 points now straddle the workspace's chunk edge at 4096
    Fb = paths(torch.as_tensor(big, device="cuda"))
    assert isinstance(Fb, torch.Tensor) and Fb.is_cuda and Fb.shape == (3, 4097)  # a device tensor in, a device tensor out
    Fb = np.roll(Fb.cpu().numpy(), -4000, axis=1)[:, :len(XT)]
    scale = np.max(np.abs(F))
    assert np.max(np.abs(Fp - F[:, perm])) <= 1e-12 * scale and np.max(np.abs(Fb - F)) <= 1e-12 * scale


def test_pitched_inputs_and_outputs(env):
    AGP, L, torch = env["AGP"], env["L"], env["torch"]
    model, Z, _ = _svgp(65)
    S, nt = 5, 70
    paths = AGP.sample_paths(model, S, n_features=63, seed=8, t=1)
    want = paths(XT[:nt])
    for (ldx, offx), (ldo, offo) in zip(layouts(3, "f64"), layouts(nt, "f64")):
        xin = Pitched("f64", data=XT[:nt], ld=ldx, off=offx, device="cuda")
        out = Pitched("f64", rows=S, width=nt, ld=ldo, off=offo, device="cuda")
        assert L.agp_pathwise_eval(paths._p, C.c_void_p(xin.ptr), ldx, nt, C.c_void_p(out.ptr), ldo) == 0
        torch.cuda.synchronize()
        xin.check("xt")
        out.check("out")
        assert not out.unwritten().any() and np.array_equal(out.window(), want)
    # the tables through padded leading dimensions
    tb = paths.tables(0)
    for which, name in ((env["capi"].PW_W, "W"), (env["capi"].PW_V, "V"), (env["capi"].PW_OMEGA, "omega")):
        r, c = tb[name].shape
        o = Pitched("f64", rows=r, width=c, ld=c + 3, off=1, device="cuda")
        assert L.agp_pathwise_get(paths._p, 0, which, C.c_void_p(o.ptr), c + 3) == 0
        torch.cuda.synchronize()
        o.check(name)
        assert np.array_equal(o.window(), tb[name])


# ---- a draw is a snapshot ----------------------------------------------------------------------------------------------------------
def _fresh_svgp(AGP):
    rng, X, f = _data(300)
    y = np.sign(f + 0.3 * rng.standard_normal(len(X)))
    model = AGP.SVGP(_kernel(AGP), AGP.LogisticLikelihood(), AGP.AnalyticSVI(50), rng.standard_normal((64, 3)), optimiser=False, seed=1)
    AGP.train_(model, X, y, 5)
    return model, X, y


def test_snapshot_survives_training_set_kernel_and_the_handle(env):
    AGP, L = env["AGP"], env["L"]
    model, X, y = _fresh_svgp(AGP)
    paths = AGP.sample_paths(model, 4, n_features=65, seed=31, t=2)
    F0, T0 = paths(XT), paths.tables(0)
    AGP.train_(model, X, y, 3)
    assert np.array_equal(paths(XT), F0)
    kd, keep = _kernel(AGP, "matern32", 0.7, 2.0).desc(3)
    model._chk(L.agp_svgp_set_kernel(model._h, 0, C.byref(kd)))
    model._chk(L.agp_svgp_refresh_K(model._h))
    assert np.array_equal(paths(XT), F0)
    L.agp_svgp_destroy(model._h)
    model._h = None
    assert np.array_equal(paths(XT), F0)
    assert all(np.array_equal(T0[k], v) for k, v in paths.tables(0).items())
    # the same (seed, t) on a fresh handle: the same tables; another t: other tables
    other, _, _ = _fresh_svgp(AGP)
    same, diff = AGP.sample_paths(other, 4, n_features=65, seed=31, t=2), AGP.sample_paths(other, 4, n_features=65, seed=31, t=3)
    for name in ("omega", "phase", "W", "E"):
        assert np.array_equal(same.tables(0)[name], T0[name]), name
        assert not np.array_equal(diff.tables(0)[name], T0[name]), name
    paths.free()
    paths.free()  # idempotent
    with pytest.raises(RuntimeError, match="freed"):
        paths(XT)


def test_seed_none_takes_the_models_seed(env):
    AGP = env["AGP"]
    model, Z, _ = _svgp(63)
    a = AGP.sample_paths(model, 2, n_features=8)
    b = AGP.sample_paths(model, 2, n_features=8)
    assert a.seed == b.seed == model.seed and np.array_equal(a.tables(0)["W"], b.tables(0)["W"])


# ---- refusals and limits through the ABI -------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A


def _draw_status(L, h, nf=8, S=2, seed=1, t=0, out=True):
    p = C.c_void_p(SENTINEL)
    st = L.agp_svgp_pathwise_draw(h, nf, S, C.c_uint64(seed), t, C.byref(p) if out else None)
    return st, p.value


def test_refused_handles_by_name(env):
    AGP, L, capi = env["AGP"], env["L"], env["capi"]
    rng = np.random.default_rng(0)
    X = rng.random((20, 2))
    y = np.sign(X[:, 0] - 0.5)
    Z = X[:5].copy()
    k = AGP.SqExponentialKernel()
    two = [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)]
    sharded = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z)
    cases = {
        "AGP_F32": AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z, T=np.float32),
        "MOSVGP": AGP.MOSVGP(k, two, AGP.AnalyticVI(), [Z, Z]),
        "MOVGP": AGP.MOVGP(X, [y, X[:, 1]], k, two, AGP.AnalyticVI(), 2),
        "AGP_FLAG_SAMPLED": AGP.MCGP(X, y, k, AGP.LogisticLikelihood(), AGP.GibbsSampling()),
        "AGP_FLAG_NUMERICAL": AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.QuadratureVI(), Z, optimiser=False),
        "follow-up": AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.QuadratureVI(), optimiser=False),
        "AGP_FLAG_MC": AGP.SVGP(k, AGP.SoftMaxLikelihood(3), AGP.MCIntegrationVI(nMC=10, seed=1), Z, optimiser=False),
        "latent-sharded": AGP.SVGP(k, AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(10), Z, latent_slice=(1, 3)),
        "batch-sharded": sharded,
    }
    for word, model in cases.items():
        h = model._ensure_handle(20)
        if model is sharded:
            model._chk(L.agp_svgp_set_batch_shard(h, 0, 2))
        before = [np.asarray(a).copy() for a in model.get_state(0)]
        st, p = _draw_status(L, h)
        msg = L.agp_last_error(model._ctx).decode()
        assert st == 5 and p == SENTINEL and word in msg, (word, st, msg)
        assert all(np.array_equal(a, b) for a, b in zip(before, model.get_state(0))), word


def test_argument_limits(env):
    AGP, L, ctx, torch = env["AGP"], env["L"], env["ctx"], env["torch"]
    model, Z, _ = _svgp(63)
    h = model._h
    before = [a.copy() for a in model.get_state(0)]
    for kw in (dict(nf=0), dict(nf=65537), dict(S=0), dict(S=65537), dict(nf=65536, S=65536), dict(t=-1), dict(t=2 ** 32), dict(out=False)):
        st, p = _draw_status(L, h, **kw)
        assert st == 1 and p == SENTINEL and L.agp_last_error(model._ctx), kw
    assert all(np.array_equal(a, b) for a, b in zip(before, model.get_state(0)))
    # the spectral draw alone: n_features * D at 2^32, t out of range, a kernel that is none of the four
    kd, keep = _kernel(AGP).desc(3)
    om = torch.full((4, 3), 7.0, dtype=torch.float64, device="cuda")
    ph = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    args = (C.c_void_p(om.data_ptr()), C.c_void_p(ph.data_ptr()))
    assert L.agp_pathwise_features(ctx, C.byref(kd), 65536, 65536, C.c_uint64(1), 0, 0, *args) == 1
    assert L.agp_pathwise_features(ctx, C.byref(kd), 3, 4, C.c_uint64(1), 2 ** 32, 0, *args) == 1
    assert L.agp_pathwise_features(ctx, C.byref(kd), 3, 4, C.c_uint64(1), 0, -1, *args) == 1
    assert L.agp_pathwise_features(ctx, C.byref(kd), 3, 4, C.c_uint64(1), 0, 0, None, args[1]) == 1
    kd.kind = 7
    assert L.agp_pathwise_features(ctx, C.byref(kd), 3, 4, C.c_uint64(1), 0, 0, *args) == 1
    torch.cuda.synchronize()
    assert bool((om == 7.0).all()) and bool((ph == 7.0).all())
    # evaluation and table export
    paths = AGP.sample_paths(model, 2, n_features=8, seed=1)
    xt = torch.as_tensor(XT[:10], device="cuda").contiguous()
    out = torch.full((2, 10), 7.0, dtype=torch.float64, device="cuda")
    px, po = C.c_void_p(xt.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.agp_pathwise_eval(paths._p, px, 2, 10, po, 10) == 1   # ldx < D
    assert L.agp_pathwise_eval(paths._p, px, 3, 10, po, 9) == 1    # ldo < n_t
    assert L.agp_pathwise_eval(paths._p, None, 3, 10, po, 10) == 1
    assert L.agp_pathwise_eval(paths._p, px, 3, 10, None, 10) == 1
    assert L.agp_pathwise_eval(paths._p, px, 3, -1, po, 10) == 1
    assert L.agp_pathwise_eval(paths._p, None, 0, 0, None, 0) == 0  # n_t = 0: a successful no-op
    assert L.agp_pathwise_get(paths._p, 0, env["capi"].PW_W, po, 1) == 1  # ld < S
    assert L.agp_pathwise_get(paths._p, 1, env["capi"].PW_W, po, 2) == 1  # no such latent
    assert L.agp_pathwise_get(paths._p, 0, 9, po, 2) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert paths(np.empty((0, 3))).shape == (2, 0)
    info = (C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64())
    assert L.agp_pathwise_info(paths._p, *[C.byref(v) for v in info]) == 0
    assert [v.value for v in info] == [1, 8, 2, 63, 3]
