"""QuadratureVI -- VGP(X, y, kernel, likelihood, QuadratureVI()) and SVGP(kernel, likelihood, QuadratureVI() / QuadratureSVI(B), Z)
(src/inference/numericalVI.jl, src/inference/quadratureVI.jl) -- and MCIntegrationVI / MCIntegrationSVI on the same two models for the
multi-class likelihoods SoftMax and LogisticSoftMax (src/inference/MCVI.jl): K latents, each with the single latent's step.

The inference objects (QuadratureVI, QuadratureSVI, NumericalVI, NumericalSVI) live in svgp.py next to AnalyticVI; the models are
SVGP and VGP themselves, whose device handle is created with AGP_FLAG_NUMERICAL (VGP: | AGP_FLAG_FULL) and keeps (mu, Sigma) and
the optimiser's moments.  This module holds what is specific to the numerical path: the Gauss-Hermite rule the host hands to the device, the
training loop (agp_svgp_nvi_step), the optimiser state for save / load, and the quadrature kernel on given moments
(quad_expectations).  include/agp_hip.h, "NUMERICAL INFERENCE", states the step and the three definitions of the reference that are
restated in their intended form.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional

import numpy as np

from . import capi
from .svgp import ADAM, Descent, Momentum, State


def gauss_hermite_rule(n: int):
    """(x, w): x_j = sqrt(2) t_j, w_j = omega_j / sqrt(pi) with (t, omega) the n-point Gauss-Hermite rule (quadratureVI.jl:36-40), so
    that E_{N(mu, s2)}[phi(f)] ~ sum_j w_j phi(mu + sqrt(s2) x_j).  The arrays are what the device receives, bit for bit."""
    t, om = np.polynomial.hermite.hermgauss(int(n))
    return np.ascontiguousarray(t * math.sqrt(2.0)), np.ascontiguousarray(om / math.sqrt(math.pi))


def rule_args(o):
    """(opt_kind, eta, p1, p2, eps) of agp_svgp_nvi_configure for an optimiser object"""
    if isinstance(o, Descent):
        return capi.OPT_DESCENT, o.eta, 0.0, 0.0, 0.0
    if isinstance(o, Momentum):
        return capi.OPT_MOMENTUM, o.eta, o.rho, 0.0, 0.0
    if isinstance(o, ADAM):
        return capi.OPT_ADAM, o.eta, o.beta[0], o.beta[1], o.eps
    raise NotImplementedError("QuadratureVI: the optimisers on the device are Descent, Momentum and ADAM")


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def configure(model, h) -> None:
    """install the quadrature rule and the optimiser of model.inference on a fresh handle"""
    inf = model.inference
    kind, eta, p1, p2, eps = rule_args(inf.nvi_optimiser)
    if getattr(inf, "mc", False):  # MCIntegrationVI: the number of draws and the seed of the table instead of a rule
        return model._chk(capi.lib().agp_svgp_mcvi_configure(h, inf.nMC, inf.seed, 1 if inf.natural else 0, kind, eta, p1, p2, eps))
    x, w = gauss_hermite_rule(inf.nGaussHermite)
    model._chk(capi.lib().agp_svgp_nvi_configure(h, len(x), _dptr(x), _dptr(w), 1 if inf.natural else 0, kind, eta, p1, p2, eps))


def nvi_info(model, latent: int = 0):
    """(alpha of the last step, halvings, rejected updates) of one latent of the handle since it was created"""
    a, hv, rj = C.c_double(), C.c_int64(), C.c_int64()
    model._chk(capi.lib().agp_svgp_nvi_info(model._h, int(latent), C.byref(a), C.byref(hv), C.byref(rj)))
    return a.value, int(hv.value), int(rj.value)


def get_opt_state(model, latent: int = 0):
    """(mom_mu [2, N], mom_sigma [2, N, N], t): the optimiser's moments of mu and Sigma of one latent and the step counter (one for
    all latents)"""
    import torch

    N, dev = model.m, model._dev()
    mm = torch.empty(2, N, dtype=torch.float64, device=dev)
    ms = torch.empty(2, N, N, dtype=torch.float64, device=dev)
    t = C.c_int64()
    model._chk(capi.lib().agp_svgp_nvi_state(model._h, int(latent), 0, C.c_void_p(mm.data_ptr()), C.c_void_p(ms.data_ptr()),
                                             C.byref(t)))
    model._chk(capi.lib().agp_ctx_sync(model._ctx))
    return mm.cpu().numpy(), ms.cpu().numpy(), int(t.value)


def set_opt_state(model, mom_mu, mom_sigma, t: int, latent: int = 0) -> None:
    import torch

    N, dev = model.m, model._dev()
    mm = torch.as_tensor(np.asarray(mom_mu, dtype=np.float64), device=dev).contiguous()
    ms = torch.as_tensor(np.asarray(mom_sigma, dtype=np.float64), device=dev).contiguous()
    if tuple(mm.shape) != (2, N) or tuple(ms.shape) != (2, N, N):
        raise ValueError("the optimiser state is (2, N) for mu and (2, N, N) for Sigma")
    model._chk(capi.lib().agp_svgp_nvi_state(model._h, int(latent), 1, C.c_void_p(mm.data_ptr()), C.c_void_p(ms.data_ptr()),
                                             C.byref(C.c_int64(int(t)))))
    model._chk(capi.lib().agp_ctx_sync(model._ctx))


def train_numerical(model, iterations: int, *, X=None, y=None, callback: Optional[Callable] = None, state: Optional[State] = None,
                    obsdim: int = 1, idx_stream=None):
    """train!(model, [X, y,] iterations) with QuadratureVI / QuadratureSVI  training.jl:13-111 with variational_updates of
    numericalVI.jl:101-119: a fixed number of steps; a VGP on its own data, an SVGP on (X, y) with minibatches of
    inference.batchsize drawn like AnalyticSVI's (or taken from idx_stream).  Without `state` the optimiser starts anew (init_state,
    states.jl:50-84), as in the reference; `state=` continues it.  alpha of every step is appended to model.nvi_alphas: a float, or
    with MCIntegrationVI the K-tuple of the latents' alphas."""
    import torch

    L = capi.lib()
    if not iterations > 0:
        raise ValueError("Number of iterations should be positive")
    inf = model.inference
    full = X is None
    Xd = model._upload(model.X if full else X, 1 if full else obsdim)
    yt = model._treat(model.y if full else y)
    N = Xd.shape[0]
    if len(yt) != N:
        raise ValueError(f"There is not the same number of samples in X ({N}) and y ({len(yt)})")
    yd = model._upload_y(yt)
    if inf.stoch:
        if not (0 < inf.batchsize <= N):
            raise ValueError(f"The size of mini-batch {inf.batchsize} is incorrect (negative or bigger than number "
                             "of samples), please set `batchsize` correctly in the inference object")
        inf.rho = N / inf.batchsize
    else:
        inf.batchsize, inf.rho = N, 1.0
    B = inf.batchsize
    h = model._ensure_handle(B)
    model._data = (Xd, yd, N)
    model._last_idx = None
    if not hasattr(model, "nvi_alphas"):
        model.nvi_alphas = []
    if state is None:
        model._chk(L.agp_svgp_init_state(h))
    else:
        model._chk(L.agp_svgp_invalidate_data(h))
    model._chk(L.agp_svgp_refresh_K(h))
    a = C.c_double()
    for it in range(1, iterations + 1):
        idx_ptr = None
        if inf.stoch:  # StatsBase.sample(1:N, B; replace=false)  training.jl:51-53 (or the caller's stream)
            if idx_stream is not None:
                idx_np = np.asarray(idx_stream[it - 1], dtype=np.int64)
                if idx_np.shape != (B,):
                    raise ValueError("idx_stream entries must have length batchsize")
            else:
                idx_np = model.rng.choice(N, B, replace=False).astype(np.int64)
            idx = torch.as_tensor(idx_np, device=model._dev())
            model._keep = [idx]
            idx_ptr = C.c_void_p(idx.data_ptr())
        model._chk(L.agp_svgp_nvi_step(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), idx_ptr, B, inf.rho))
        model._last_idx = idx_ptr
        if getattr(inf, "mc", False):
            al = []
            for k in range(model.n_latent):
                model._chk(L.agp_svgp_nvi_info(h, k, C.byref(a), None, None))
                al.append(a.value)
            model.nvi_alphas.append(tuple(al))
        else:
            model._chk(L.agp_svgp_nvi_info(h, 0, C.byref(a), None, None))
            model.nvi_alphas.append(a.value)
        model.trained = True
        if callback is not None:
            callback(model, State(model), inf.n_iter)
        if model.verbose > 2 or (model.verbose > 1 and it % 10 == 0):
            from .svgp import objective

            print(f"iter {it}  ELBO {objective(model, State(model), None):.6f}")
        inf.n_iter += 1
    if model.verbose > 0:
        print(f"Training ended after {iterations} iterations. Total number of iterations {inf.n_iter}")
    model._chk(L.agp_svgp_check_status(h))
    model._chk(L.agp_svgp_refresh_K(h))
    return model, State(model)


def quad_expectations(likelihood, y, mu, var, nodes, weights, *, device: Optional[int] = None):
    """(ell, g, h): sum_j w_j l(y_i, f_ij), sum_j w_j l'(y_i, f_ij), sum_j w_j l''(y_i, f_ij) at f_ij = mu_i + sqrt(max(var_i, 0)) x_j
    for the Logistic, StudentT and Laplace (h in closed form) likelihoods -- the quadrature kernel on given moments, outside any
    model (agp_quad_expectations)."""
    import torch

    L = capi.lib()
    dev = torch.device("cuda", device if device is not None else torch.cuda.current_device())
    yt, mt, vt = (torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev).contiguous() for a in (y, mu, var))
    if not (yt.ndim == 1 and yt.shape == mt.shape == vt.shape):
        raise ValueError("y, mu and var are vectors of one length")
    x = np.ascontiguousarray(nodes, dtype=np.float64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if x.ndim != 1 or x.shape != w.shape:
        raise ValueError("nodes and weights are vectors of one length")
    ctx = C.c_void_p()
    st = L.agp_ctx_create(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(ctx))
    if st != capi.AGP_OK:
        raise capi.AGPError(st, "agp_ctx_create failed")
    try:
        ell, g, h = torch.empty_like(yt), torch.empty_like(yt), torch.empty_like(yt)
        d = likelihood.lik_desc()
        capi.check(ctx, L.agp_quad_expectations(ctx, C.byref(d), C.c_void_p(yt.data_ptr()), C.c_void_p(mt.data_ptr()),
                                                C.c_void_p(vt.data_ptr()), yt.numel(), _dptr(x), _dptr(w), len(x),
                                                C.c_void_p(ell.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(h.data_ptr())))
        return ell.cpu().numpy(), g.cpu().numpy(), h.cpu().numpy()
    finally:
        L.agp_ctx_destroy(ctx)


def _ctx_call(device, fn):
    """run fn(L, ctx, dev) on a context of its own (the two context-level entry points below)"""
    import torch

    L = capi.lib()
    dev = torch.device("cuda", device if device is not None else torch.cuda.current_device())
    ctx = C.c_void_p()
    st = L.agp_ctx_create(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(ctx))
    if st != capi.AGP_OK:
        raise capi.AGPError(st, "agp_ctx_create failed")
    try:
        return fn(L, ctx, dev)
    finally:
        L.agp_ctx_destroy(ctx)


def mc_normals(seed: int, t: int, stream: int, nMC: int, K: int, *, device: Optional[int] = None):
    """the table eps[nMC, K] of standard normals of (seed, t, stream) as the device draws it (agp_mc_normals): stream 2 is the
    gradient draw of step t, stream 3 the draw of an ELBO evaluated after t steps (include/agp_hip.h, "MC INTEGRATION")"""
    import torch

    def run(L, ctx, dev):
        out = torch.empty(int(nMC), int(K), dtype=torch.float64, device=dev)
        capi.check(ctx, L.agp_mc_normals(ctx, int(seed), int(t), int(stream), int(nMC), int(K), C.c_void_p(out.data_ptr())))
        return out.cpu().numpy()

    return _ctx_call(device, run)


def mc_expectations(likelihood, y_class, mu, var, nMC: int, seed: int, t: int, stream: int = 2, *, device: Optional[int] = None):
    """(ell [n], g [K, n], h [K, n]): the means over the nMC draws of log p(c_i | f), d log p / d f_k and d2 log p / d f_k^2 at
    f_sk = mu_ki + sqrt(max(var_ki, 0)) eps_sk for the SoftMax and LogisticSoftMax likelihoods -- the expectation kernel on given
    moments, outside any model (agp_mc_expectations).  y_class: 0-based class indices [n]; mu, var: [K, n]."""
    import torch

    def run(L, ctx, dev):
        yt = torch.as_tensor(np.asarray(y_class, dtype=np.int32), device=dev).contiguous()
        mt, vt = (torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev).contiguous() for a in (mu, var))
        if not (yt.ndim == 1 and mt.ndim == 2 and mt.shape == vt.shape and mt.shape[1] == yt.shape[0]):
            raise ValueError("y_class is a vector of n class indices, mu and var are (K, n)")
        K, n = mt.shape
        ell = torch.empty(n, dtype=torch.float64, device=dev)
        g, h = torch.empty_like(mt), torch.empty_like(mt)
        d = likelihood.lik_desc()
        capi.check(ctx, L.agp_mc_expectations(ctx, C.byref(d), C.c_void_p(yt.data_ptr()), C.c_void_p(mt.data_ptr()),
                                              C.c_void_p(vt.data_ptr()), n, K, int(nMC), int(seed), int(t), int(stream),
                                              C.c_void_p(ell.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(h.data_ptr())))
        return ell.cpu().numpy(), g.cpu().numpy(), h.cpu().numpy()

    return _ctx_call(device, run)
