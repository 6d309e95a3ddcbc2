"""Input gradients of the predictive moments: d mu(x*) / d x* and d sigma^2(x*) / d x* of what predict_f returns, on the device over
any number of test points (agp_svgp_predict_f_grad; include/agp_hip.h, "PREDICTIVE GRADIENTS").  What gradient
ascent on an acquisition function (UCB, EI), sensitivity analysis and mode finding need, without finite differences of predict_f.
No counterpart in the reference.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

from . import capi
from .mcgp import MCGP
from .online import OnlineSVGP
from .svgp import MOSVGP, SVGP

MAX_D = 64  # the limit of the hyper-gradient (agp_hip.h), for the same reason


def predgrad_refusal(model) -> Optional[str]:
    """Why agp_svgp_predict_f_grad refuses this model, or None: decided here, before the device is touched."""
    if isinstance(model, OnlineSVGP):
        if model._cur is None:
            return "the online model has not seen a batch yet"
        model = model._cur
    if not isinstance(model, SVGP):
        return f"{type(model).__name__} is not a model with a device handle (SVGP, MOSVGP, VGP, GP, MOVGP, OnlineSVGP)"
    if isinstance(model, MCGP) or getattr(model, "_desc_flags", 0) & capi.FLAG_SAMPLED:
        return "Gibbs-sampled models (MCGP) are not supported: they have no predict_f to differentiate"
    for k in model.kernels:
        if k._kind == capi.K_EXPONENTIAL:
            return "ExponentialKernel is not differentiable at zero distance"
    if model.D > MAX_D:
        return f"the input dimension D = {model.D} exceeds {MAX_D} (the limit of the hyper-gradient)"
    if getattr(model, "latent_offset", 0) != 0 or getattr(model, "n_latent_total", model.n_latent) != model.n_latent:
        return "latent-sharded models (latent_slice) are not supported"
    if getattr(model, "_batch_shard", None) is not None and model._batch_shard[1] > 1:
        return "batch-sharded models are not supported"
    return None


def _grad_svgp(model: SVGP, X_test, cov: bool, obsdim: int):
    if not isinstance(cov, bool):
        raise TypeError("predict_f_grad: cov is a bool")
    if obsdim not in (1, 2):
        raise ValueError("predict_f_grad: obsdim is 1 (points are rows) or 2 (points are columns)")
    why = predgrad_refusal(model)
    if why is not None:
        raise NotImplementedError(f"predict_f_grad: {why}")
    import torch

    L = capi.lib()
    Xd = model._upload(X_test, obsdim)
    nt, D = Xd.shape
    h = model._ensure_handle(max(model._max_batch, 1))
    dev = model._dev()
    dmu = torch.empty(model.n_out, nt, D, dtype=model.tdtype, device=dev)
    dvar = torch.empty(model.n_out, nt, D, dtype=model.tdtype, device=dev) if cov else None
    model._chk(L.agp_svgp_predict_f_grad(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), nt, C.c_void_p(dmu.data_ptr()),
                                         C.c_void_p(dvar.data_ptr()) if cov else None, D))
    model._chk(L.agp_ctx_sync(model._ctx))
    gm = dmu.cpu().numpy()
    gv = dvar.cpu().numpy() if cov else None
    if model.n_out > 1 or isinstance(model, MOSVGP):  # predict_f's conventions: a tuple over latents / tasks
        gm = tuple(gm[k] for k in range(model.n_out))
        return (gm, tuple(gv[k] for k in range(model.n_out))) if cov else gm
    return (gm[0], gv[0]) if cov else gm[0]


@functools.singledispatch
def predict_f_grad(model, X_test, *, cov: bool = True, obsdim: int = 1):
    """(dmu, dvar): the gradients of predict_f(model, X_test, cov=True) with respect to the test inputs, (n_t, D) arrays
    (dmu[i, d] = d mu(x_i) / d x_id); dmu alone with cov=False (the variance path is then not run at all).  Several latents
    (LogisticSoftMax, Heteroscedastic) or tasks (MOSVGP, MOVGP: the mixed outputs): tuples over them, as predict_f returns.
    SqExponential, Matern32 and Matern52 kernels with ScaleTransform / ARDTransform, D <= 64; a test point that coincides with an
    inducing point is an ordinary input.  Streamed in chunks of 4096 points, deterministic, and the model's state is left as it was.
    SVGP (AnalyticVI / SVI, QuadratureVI, MCIntegrationVI), MOSVGP, VGP, GP, MOVGP, OnlineSVGP; an MCGP, the ExponentialKernel and
    D > 64 raise NotImplementedError before the device is touched."""
    raise NotImplementedError(f"predict_f_grad: {predgrad_refusal(model)}")


@predict_f_grad.register(SVGP)  # MOSVGP, VGP, GP and MOVGP are SVGPs
def _(model, X_test, *, cov: bool = True, obsdim: int = 1):
    return _grad_svgp(model, X_test, cov, obsdim)


@predict_f_grad.register(MCGP)
def _(model, X_test, *, cov: bool = True, obsdim: int = 1):
    raise NotImplementedError(f"predict_f_grad: {predgrad_refusal(model)}")


@predict_f_grad.register(OnlineSVGP)
def _(model, X_test, *, cov: bool = True, obsdim: int = 1):
    why = predgrad_refusal(model)
    if why is not None:
        raise NotImplementedError(f"predict_f_grad: {why}")
    return _grad_svgp(model._cur, X_test, cov, obsdim)
