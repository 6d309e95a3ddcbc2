"""predict_f_grad without a GPU: the NumPy restatement of the gradients (tests/_predgrad_ref.py) against torch autograd through the
oracle's predict_f; the conditioning of every GPU parity case (tests/_predgrad_cases.py); the host mirror's refusals and argument
checks, which are decided before the device is touched; the entry point in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

import _predgrad_cases as PC
import _predgrad_ref as G
from oracle import agp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement is the gradient of the oracle's predict_f ------------------------------------------------------------------
def _torch_phi(kind, q):
    if kind == "sqexponential":
        return torch.exp(-q / 2)
    # sqrt has no derivative at 0: a coinciding pair enters through its limit, phi = 1 with zero gradient (phi is even and smooth in
    # the difference for the two Matern kernels used here)
    pos = q > 0
    r = torch.sqrt(torch.where(pos, q, torch.ones_like(q)))
    r = torch.where(pos, r, torch.zeros_like(q))
    if kind == "matern32":
        return (1 + np.sqrt(3.0) * r) * torch.exp(-np.sqrt(3.0) * r)
    return (1 + np.sqrt(5.0) * r + 5 * q / 3) * torch.exp(-np.sqrt(5.0) * r)


def _torch_predict_f(x, kernel, Z, a, A, jitter):
    """SVGP.predict_f of oracle/agp_ref.py (mu = k* K^-1 mu, var = k** + jitt - k* A k*') for ONE point x, as a torch function"""
    s = torch.as_tensor(np.broadcast_to(np.asarray(kernel.scale, dtype=np.float64), (Z.shape[1],)).copy())
    diff = (x[None, :] - torch.as_tensor(Z)) * s[None, :]
    ks = kernel.sigma2 * _torch_phi(kernel.kind, torch.sum(diff * diff, dim=1))
    return ks @ torch.as_tensor(a), kernel.sigma2 + jitter - ks @ (torch.as_tensor(A) @ ks)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("ard", [False, True])
def test_restatement_is_the_gradient_of_the_oracle_predict_f(kind, ard):
    rng = np.random.default_rng(5 + len(kind) + ard)
    m, D, N = 40, 3, 200
    X = rng.standard_normal((N, D))
    y = np.sign(np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] + 0.2 * rng.standard_normal(N))
    Z = X[:m].copy()
    kernel = R.Kernel(kind, np.array([1.5, 2.5, 0.8]) if ard else 2.0, 1.5)
    ref = R.SVGP(kernel, R.LogisticLikelihood(), Z, stochastic=True, batchsize=50)
    ref.train(X, y, 4, idx_stream=[rng.choice(N, 50, replace=False) for _ in range(4)])
    gp = ref.latents[0]
    parts = G.latent_parts(gp.kernel, gp.Z, gp.L, gp.mu, gp.Sigma)
    Xt = np.vstack([rng.standard_normal((12, D)), Z[:5]])  # the last five ARE inducing points
    # the restated moments are the oracle's
    mu_r, var_r = ref.predict_f(Xt, cov=True)
    mu_g, var_g = G.moments(Xt, *parts, jitter=ref.jitter)
    assert G.rel(mu_g, mu_r[0]) < 1e-12 and G.rel(var_g, var_r[0]) < 1e-10
    dmu, dvar = G.grads(Xt, *parts)
    am, av = np.empty_like(dmu), np.empty_like(dvar)
    for i, x in enumerate(Xt):
        for out, which in ((am, 0), (av, 1)):
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            _torch_predict_f(xt, gp.kernel, gp.Z, parts[4], parts[5], ref.jitter)[which].backward()
            out[i] = xt.grad.numpy()
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    em, ev = G.rel(dmu, am), G.rel(dvar, av)
    print(f"{kind} ard={ard}: restatement against autograd  dmu {em:.2e}  dvar {ev:.2e}")
    assert em < 1e-10 and ev < 1e-10


def test_coinciding_point_adds_exactly_zero():
    """x = z_j: that j's term is exactly 0 in the restatement, for every kernel (nothing divides by r)"""
    Z = np.array([[0.3, -1.2], [2.0, 0.5]])
    for kind in G.KINDS:
        dmu, dvar = G.grads(Z[:1], Z[:1], 1.7, 1.5, kind, np.array([3.0]), np.array([[2.0]]))
        assert np.all(dmu == 0.0) and np.all(dvar == 0.0)
        dmu, _ = G.grads(Z[:1], Z, 1.7, 1.5, kind, np.array([3.0, 1.0]))
        only, _ = G.grads(Z[:1], Z[1:], 1.7, 1.5, kind, np.array([1.0]))
        assert np.array_equal(dmu, only)


# ---- every GPU parity case is well conditioned: a condition on the INPUTS (change the case, not the bound) -------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_case_is_well_conditioned(name):
    gm, gv = PC.restated(name, np.float64)
    hm, hv = PC.restated(name, np.longdouble)
    assert len(gm) == len(hm) == len(gv) == len(hv) >= 1
    for k in range(len(gm)):
        em, ev = G.rel(gm[k], hm[k]), G.rel(gv[k], hv[k])
        print(f"{name}[{k}]: float64 against longdouble  dmu {em:.2e}  dvar {ev:.2e}   max |dmu| {np.max(np.abs(gm[k])):.2e}  "
              f"max |dvar| {np.max(np.abs(gv[k])):.2e}")
        assert gm[k].shape == (PC.CASES[name]["nt"], PC.CASES[name]["D"])
        assert np.max(np.abs(gm[k])) > 1e-3 and np.max(np.abs(gv[k])) > 1e-3  # (not a comparison of zeros)
        assert em < 1e-10 and ev < 1e-10


def test_cases_cover_the_axes():
    ms = {c["m"] for c in PC.CASES.values()}
    assert {1, 63, 64, 65, 130} <= ms
    assert {c["D"] for c in PC.CASES.values()} >= {1, 3, 64}
    assert {c["nt"] for c in PC.CASES.values()} >= {1, 255, 4096 + 37}
    kt = {(c["kind"], np.isscalar(c["scale"])) for c in PC.CASES.values()}
    assert kt >= {(k, s) for k in G.KINDS for s in (True, False)}
    assert {c["model"] for c in PC.CASES.values()} == {"svgp", "mosvgp", "vgp", "gp", "quad", "online"}


# ---- refusals and argument checks of the host mirror: before the device is touched -------------------------------------------------
def _svgp(AGP, kernel=None, D=3, m=5, **kw):
    Z = np.random.default_rng(0).standard_normal((m, D))
    return AGP.SVGP(kernel or AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.AnalyticVI(), Z, optimiser=False, **kw)


def test_python_refusals():
    import agp_amd as AGP
    from agp_amd.predgrad import predgrad_refusal

    X = np.zeros((4, 3))
    assert predgrad_refusal(_svgp(AGP)) is None
    with pytest.raises(NotImplementedError, match="ExponentialKernel is not differentiable"):
        AGP.predict_f_grad(_svgp(AGP, AGP.ExponentialKernel()), X)
    with pytest.raises(NotImplementedError, match="exceeds 64"):
        AGP.predict_f_grad(_svgp(AGP, D=65), np.zeros((4, 65)))
    assert predgrad_refusal(_svgp(AGP, D=64)) is None
    rng = np.random.default_rng(1)
    Xn = rng.standard_normal((6, 2))
    mc = AGP.MCGP(Xn, np.sign(Xn[:, 0]), AGP.SqExponentialKernel(), AGP.LogisticLikelihood(), AGP.GibbsSampling())
    with pytest.raises(NotImplementedError, match="MCGP"):
        AGP.predict_f_grad(mc, Xn)
    with pytest.raises(NotImplementedError, match="latent-sharded"):
        AGP.predict_f_grad(AGP.SVGP(AGP.SqExponentialKernel(), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticVI(), np.zeros((4, 3)),
                                    optimiser=False, latent_slice=(0, 2)), X)
    on = AGP.OnlineSVGP(AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), optimiser=False)
    with pytest.raises(NotImplementedError, match="not seen a batch"):
        AGP.predict_f_grad(on, X)
    with pytest.raises(NotImplementedError, match="not a model"):
        AGP.predict_f_grad(object(), X)


def test_python_argument_checks():
    import agp_amd as AGP

    model = _svgp(AGP)
    with pytest.raises(TypeError, match="cov is a bool"):
        AGP.predict_f_grad(model, np.zeros((4, 3)), cov=1)
    with pytest.raises(ValueError, match="obsdim"):
        AGP.predict_f_grad(model, np.zeros((4, 3)), obsdim=3)
    for cls in ("SVGP", "MOSVGP", "VGP", "GP", "MOVGP", "OnlineSVGP", "MCGP"):
        assert AGP.predict_f_grad.dispatch(getattr(AGP, cls)) is not AGP.predict_f_grad.dispatch(object), cls


def test_symbol_is_in_the_header_and_the_binding():
    from agp_amd import capi

    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    m = re.search(r"agp_status\s+agp_svgp_predict_f_grad\s*\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", h, flags=re.S))
    assert m, "agp_svgp_predict_f_grad is not declared in include/agp_hip.h"
    assert len(m.group(1).split(",")) == 7
    ret, args = capi.SYMBOLS["agp_svgp_predict_f_grad"]
    assert len(args) == 7
    assert "PREDICTIVE GRADIENTS" in h and "agp_svgp_predict_f_grad" in open(os.path.join(ROOT, "julia", "AGPHip.jl")).read()
