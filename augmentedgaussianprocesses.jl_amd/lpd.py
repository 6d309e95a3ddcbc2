"""Log predictive density: sum_i log p(y_i | x_i, model), the held-out log-likelihood (its negative mean is the NLPD), evaluated on
the device over any number of test points (agp_svgp_lpd_stream), and the point-wise kernel on given moments outside any model
(agp_log_predictive).  include/agp_hip.h, "LOG PREDICTIVE DENSITY", states the rule per likelihood; DESIGN.md section 9m has the
accuracy table of the Gauss-Hermite rule.

StudentT is the reference's density AS WRITTEN (studentt.jl:43-46, likelihoods.likelihood_value): the normalised t with nu degrees
of freedom and scale sigma / sqrt(nu), multiplied by sigma / sqrt(nu) -- the constant the quadrature inference uses.

Accuracy of the Gauss-Hermite kinds (Logistic, BayesianSVM, StudentT, Poisson, NegBinomial).  The n-node rule in f-space is the
reference's predictive rule; it is exact to rounding while the predictive spread sqrt(var_f) stays below the likelihood's width and
degrades when it far exceeds it.  Measured with 100 nodes against the integral (tests/test_lpd_host.py prints the table), absolute
error of lpd, worst over mu in {-1, 0.5, 2}, at sqrt(var_f) / width = 0.1, 1, 10:
    Logistic (width 1)                  <= 1e-4 for mu ~ 3 N(0, 1), var_f in [1e-6, 31] (measured worst 5.4e-5)
    BayesianSVM (width 1), y = 1        2.9e-4   3.0e-4   6.0e-2     (the hinge's kinks at f = -+1)
    StudentT nu = 3, sigma = 0.5        4.4e-16  4.2e-8   0.97       (width sigma, y = 0.3)
    Poisson lambda = 5 (width 1)        2.2e-16  4.4e-16  5.0e-2     (y = 2)
    NegBinomial r = 3 (width 1)         8.9e-16  4.4e-16  0.13       (y = 2)
A better StudentT rule (quadrature in the scale-mixture variable) is a follow-up.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from .likelihoods import (
    AbstractLikelihood,
    HeteroscedasticLikelihood,
    LogisticSoftMaxLikelihood,
)
from .nvi import _ctx_call, gauss_hermite_rule

_QUAD_KINDS = (capi.LIK_LOGISTIC, capi.LIK_BAYESIANSVM, capi.LIK_STUDENTT, capi.LIK_POISSON, capi.LIK_NEGBINOMIAL)
_KINDS = _QUAD_KINDS + (capi.LIK_GAUSSIAN, capi.LIK_LAPLACE, capi.LIK_LOGISTICSOFTMAX, capi.LIK_SOFTMAX)


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def lpd_refusal(model) -> Optional[str]:
    """Why agp_svgp_lpd_stream refuses this model (include/agp_hip.h, "LOG PREDICTIVE DENSITY"), or None: decided here, before the
    library is called."""
    from .svgp import SVGP, MOSVGP, _MultiOutputLikelihood

    if not isinstance(model, SVGP):
        return f"{type(model).__name__} is not a model with a device handle (SVGP, VGP, GP)"
    lik = model.likelihood
    if isinstance(model, MOSVGP) or isinstance(lik, _MultiOutputLikelihood):
        return "multi-output models (MOSVGP, MOVGP) are not supported"
    if getattr(model, "_desc_flags", 0) & capi.FLAG_SAMPLED:
        return "Gibbs-sampled models (MCGP) are not supported: they have no predict_f"
    if isinstance(lik, HeteroscedasticLikelihood):
        return "HeteroscedasticLikelihood is not supported: two latents, a nested integral (a follow-up)"
    if not isinstance(lik, AbstractLikelihood) or lik.kind not in _KINDS:
        return f"{type(lik).__name__} has no log predictive density on the device"
    if getattr(model, "latent_offset", 0) != 0 or getattr(model, "n_latent_total", model.n_latent) != model.n_latent:
        return "latent-sharded models (latent_slice) are not supported: a point's density needs every latent on one handle"
    if getattr(model, "_batch_shard", None) is not None and model._batch_shard[1] > 1:
        return "batch-sharded models are not supported"
    return None


def log_predictive_density(model, X, y, *, pointwise: bool = False, n_nodes: int = 100, obsdim: int = 1):
    """sum_i log p(y_i | x_i, model) over ANY number of test points, streamed on the device in chunks of 4096
    (agp_svgp_lpd_stream): lpd_i = log int p(y_i | f) N(f; mu_i, var_i) df with (mu_i, var_i) what predict_f(model, X, cov=True)
    returns.  Gaussian (with the model's current noise) and Laplace in closed form; Logistic, BayesianSVM, StudentT, Poisson (with the
    model's current lambda) and NegBinomial by the n_nodes-point Gauss-Hermite rule in f-space, formed as a log-sum-exp (no
    underflow); LogisticSoftMax / SoftMax by the link on the means, as proba_y.  See the module docstring for StudentT's density and
    for the accuracy of the Gauss-Hermite rule at large var_f.  Accepts SVGP, VGP, GP and models trained with QuadratureVI /
    MCIntegrationVI; labels go through the model's own treat_labels.  Deterministic: two calls return the same bits.  The model's
    state is left as it was.  pointwise=True: (sum, lpd[n])."""
    why = lpd_refusal(model)
    if why is not None:
        raise NotImplementedError(f"log_predictive_density: {why}")
    if not 1 <= int(n_nodes) <= 4096:
        raise ValueError("log_predictive_density: 1 <= n_nodes <= 4096")
    import torch

    L = capi.lib()
    Xd = model._upload(X, obsdim)
    if isinstance(y, torch.Tensor):  # (a device tensor is taken as treated labels)
        want = torch.int32 if isinstance(model.likelihood, LogisticSoftMaxLikelihood) else model.tdtype
        yd = y.to(device=model._dev(), dtype=want).contiguous()
    else:
        yd = model._upload_y(model._treat(y)).contiguous()
    n = Xd.shape[0]
    if yd.ndim != 1 or yd.shape[0] != n:
        raise ValueError(f"There is not the same number of samples in X ({n}) and y ({tuple(yd.shape)})")
    h = model._ensure_handle(max(model._max_batch, 1))
    x, w = gauss_hermite_rule(int(n_nodes))
    out = C.c_double()
    vec = torch.empty(n, dtype=model.tdtype, device=model._dev()) if pointwise else None
    model._chk(L.agp_svgp_lpd_stream(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), n, _dptr(x), _dptr(w),
                                     len(x), C.byref(out), C.c_void_p(vec.data_ptr()) if pointwise else None))
    if pointwise:
        return out.value, vec.cpu().numpy()
    return out.value


def log_predictive_moments(likelihood, y, mu, var, nodes=None, weights=None, *, dtype=np.float64, device: Optional[int] = None):
    """lpd[n]: log int p(y_i | f) N(f; mu_i, var_i) df on given moments, outside any model (agp_log_predictive) -- the point-wise
    kernel of log_predictive_density.  y, mu, var: vectors of one length; for LogisticSoftMax / SoftMax y holds 0-based class indices
    and mu, var are (K, n).  nodes, weights: the Gauss-Hermite rule (gauss_hermite_rule), not needed for Gaussian, Laplace and the
    multi-class likelihoods.  The likelihood's own parameters are used (Gaussian sigma2, Poisson lambda, ...)."""
    import torch

    if isinstance(likelihood, HeteroscedasticLikelihood) or getattr(likelihood, "kind", None) not in _KINDS:
        raise NotImplementedError(f"log_predictive_moments: {type(likelihood).__name__} has no log predictive density on the device")
    if (nodes is None) != (weights is None):
        raise ValueError("log_predictive_moments: nodes and weights come together")
    if likelihood.kind in _QUAD_KINDS and nodes is None:
        raise ValueError(f"log_predictive_moments: {type(likelihood).__name__} needs the Gauss-Hermite nodes and weights")
    x = w = None
    if nodes is not None:
        x = np.ascontiguousarray(nodes, dtype=np.float64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if x.ndim != 1 or x.shape != w.shape or not 1 <= len(x) <= 4096:
            raise ValueError("log_predictive_moments: nodes and weights are vectors of one length between 1 and 4096")
    multi = isinstance(likelihood, LogisticSoftMaxLikelihood)
    npdt = np.dtype(dtype)
    if npdt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("log_predictive_moments: dtype is float64 or float32")
    m_np, v_np = np.asarray(mu, dtype=npdt), np.asarray(var, dtype=npdt)
    y_np = np.asarray(y, dtype=np.int32 if multi else npdt)
    if multi:
        if not (y_np.ndim == 1 and m_np.ndim == 2 and m_np.shape == v_np.shape and m_np.shape[1] == y_np.shape[0]
                and m_np.shape[0] == likelihood.n_class):
            raise ValueError("log_predictive_moments: y is a vector of n class indices, mu and var are (n_class, n)")
    elif not (y_np.ndim == 1 and y_np.shape == m_np.shape == v_np.shape):
        raise ValueError("log_predictive_moments: y, mu and var are vectors of one length")
    n = y_np.shape[0]

    def run(L, ctx, dev):
        yt, mt, vt = (torch.as_tensor(a, device=dev).contiguous() for a in (y_np, m_np, v_np))
        out = torch.empty(n, dtype=mt.dtype, device=dev)
        d = likelihood.lik_desc()
        capi.check(ctx, L.agp_log_predictive(ctx, capi.F64 if npdt == np.float64 else capi.F32, C.byref(d), C.c_void_p(yt.data_ptr()),
                                             C.c_void_p(mt.data_ptr()), C.c_void_p(vt.data_ptr()), n, n,
                                             _dptr(x) if x is not None else None, _dptr(w) if w is not None else None,
                                             len(x) if x is not None else 0, C.c_void_p(out.data_ptr())))
        return out.cpu().numpy()

    return _ctx_call(device, run)
