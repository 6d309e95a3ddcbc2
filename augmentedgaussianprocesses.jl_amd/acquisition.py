"""Acquisition functions of the predictive moments and their multi-start maximiser on the device (include/agp_hip.h, "ACQUISITION
FUNCTIONS"): the other half of Bayesian optimisation next to `sample_paths`.

    a = AGP.acquisition(model, AGP.EI(best=y.max()), X)                      # (n_t,); grad=True gives (a, G (n_t, D))
    x, a = AGP.maximize_acquisition(model, AGP.UCB(2.0), X0, (lo, hi))       # the best of R ADAM ascents, on the device
    a, dmu, dvar = AGP.acquisition_moments(AGP.PI(best=0.0), mu, var, grad=True)
    Xq, aq = AGP.maximize_acquisition_batch(model, AGP.UCB(2.0), 8, X0, (lo, hi), pending=P)   # q points, greedily, on the device
    a = AGP.acquisition(model, AGP.EI(best=y.max()), X, pending=P)           # alpha with P hallucinated at its predicted mean
    Xq, aq = AGP.maximize_acquisition_joint(model, AGP.EI(best=y.max()), X0q, (lo, hi))   # q points together: Monte-Carlo q-EI
    a = AGP.acquisition_joint(model, AGP.UCB(2.0), Xq, samples=256, pending=P)            # q-UCB of the tuples (n, q, D)
    x, la = AGP.maximize_acquisition(model, AGP.LogEI(best=y.max()), X0, (lo, hi))   # log EI: no plateau far from the incumbent

UCB = s mu + beta sigma, EI = sigma (z Phi(z) + phi(z)), PI = Phi(z) with z = (s (mu - best) - xi) / sigma; s = -1 with minimize=True
(the objective is minimised; the acquisition function itself is always maximised).  EI and PI underflow to 0, with a zero gradient,
for z below about -38: an ascent that starts there does not move, and the later rounds of a batch, whose pending points shrink sigma,
are full of such starts.  LogEI = log EI and LogPI = log PI have the same maximisers and are finite with a useful gradient over the
whole range of z (the continued fraction of the Mills ratio for z <= -3: csrc/agp_acq_log.h); every returned value is then log alpha.
Float64, single-output models, D <= 64, SqExponential / Matern32 / Matern52 kernels.  Batches come from hallucinated observations
(GP-BUCB, "kriging believer"): pending points are conditioned on at their own predicted mean -- the mean stays, the variance
shrinks -- and q points are picked greedily.  Joint batches are the Monte-Carlo q-EI and q-UCB of q points under their posterior
correlation, with a joint reparameterised sample f_s = mu + L eps_s over fixed base samples (sample-average approximation) and the
sub-gradient through the winning member: `acquisition_joint`, `maximize_acquisition_joint`; there a pending point is a member of the
joint sample, not a hallucinated observation, and a greedy batch is the natural set of starts.
Not here: the joint PI and the joint log kinds, fantasies that move the mean, Float32, multi-output and sharded models.  No
counterpart in the reference.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import capi
from .pathwise import check_maximize_args
from .predgrad import MAX_D, predgrad_refusal

ACQ_UCB, ACQ_EI, ACQ_PI = 0, 1, 2
ACQ_LOG = 4  # a flag on EI and PI
ACQ_LOG_EI, ACQ_LOG_PI = ACQ_LOG | ACQ_EI, ACQ_LOG | ACQ_PI


class _Acquisition:
    kind = -1
    beta, best, xi = 0.0, 0.0, 0.0

    def check(self) -> None:
        """the argument checks of agp_acq_desc, on the host"""
        for name in ("beta", "xi"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float, np.floating, np.integer)) and math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{type(self).__name__}: {name} must be finite and >= 0 (got {v})")
        if self.best is not None and not math.isfinite(self.best):
            raise ValueError(f"{type(self).__name__}: best must be finite (got {self.best})")

    def desc(self, minimize: bool, best: Optional[float] = None) -> capi.AcqDesc:
        b = self.best if best is None else best
        return capi.AcqDesc(self.kind, int(bool(minimize)), float(self.beta), float(0.0 if b is None else b), float(self.xi))


class UCB(_Acquisition):
    """upper confidence bound s mu + beta sigma (with minimize=True the lower bound, negated: -mu + beta sigma)"""
    kind = ACQ_UCB

    def __init__(self, beta: float = 2.0):
        self.beta = beta
        self.check()

    def __repr__(self):
        return f"UCB(beta={self.beta})"


class EI(_Acquisition):
    """expected improvement over `best` by more than `xi`; best=None takes the incumbent from the model's own data (GP, VGP)"""
    kind = ACQ_EI

    def __init__(self, best: Optional[float] = None, xi: float = 0.0):
        self.best, self.xi = best, xi
        self.check()

    def __repr__(self):
        return f"EI(best={self.best}, xi={self.xi})"


class PI(_Acquisition):
    """probability of improvement over `best` by more than `xi`; best=None as for EI"""
    kind = ACQ_PI

    def __init__(self, best: Optional[float] = None, xi: float = 0.0):
        self.best, self.xi = best, xi
        self.check()

    def __repr__(self):
        return f"PI(best={self.best}, xi={self.xi})"


class LogEI(EI):
    """log EI: the maximiser of EI, finite with a useful gradient where EI has underflowed to 0 (z below about -38)"""
    kind = ACQ_LOG_EI

    def __repr__(self):
        return f"LogEI(best={self.best}, xi={self.xi})"


class LogPI(PI):
    """log PI: the maximiser of PI, finite with a useful gradient where PI has underflowed to 0"""
    kind = ACQ_LOG_PI

    def __repr__(self):
        return f"LogPI(best={self.best}, xi={self.xi})"


def acquisition_refusal(model, latent: int = 0) -> Optional[str]:
    """Why agp_svgp_acquisition / agp_svgp_acq_maximize refuse this model, or None: decided here, before the device is touched."""
    from .movgp import MOVGP
    from .online import OnlineSVGP
    from .svgp import MOSVGP, SVGP

    if isinstance(model, OnlineSVGP):
        if model._cur is None:
            return "the online model has not seen a batch yet"
        model = model._cur
    if isinstance(model, (MOSVGP, MOVGP)):
        return "multi-output models (MOSVGP, MOVGP) are not supported"
    why = predgrad_refusal(model)  # no handle, MCGP, ExponentialKernel (any latent), D > 64, shards
    if why is not None:
        return why
    assert isinstance(model, SVGP) and model.D <= MAX_D
    if np.dtype(model.T) != np.dtype(np.float64):
        return "Float32 models are not supported (the acquisition functions are Float64)"
    return None


def _resolve(model, acq, latent, minimize):
    """(the model that owns the handle, the checked descriptor): every refusal and argument check, before the device is touched"""
    from .gp import GP
    from .online import OnlineSVGP
    from .vgp import VGP

    if not isinstance(acq, _Acquisition):
        raise TypeError("acq must be UCB(...), EI(...), PI(...), LogEI(...) or LogPI(...)")
    acq.check()
    why = acquisition_refusal(model, latent)
    if why is not None:
        raise NotImplementedError(f"acquisition: {why}")
    if isinstance(model, OnlineSVGP):
        model = model._cur
    if not 0 <= int(latent) < model.n_latent:
        raise ValueError(f"latent must lie in [0, {model.n_latent}) (got {latent})")
    best = None
    if acq.kind != ACQ_UCB and acq.best is None:
        if not isinstance(model, (GP, VGP)) or getattr(model, "X", None) is None:
            raise ValueError(f"{type(acq).__name__}(best=None) takes the incumbent from the model's training inputs: only a GP or VGP "
                             f"has them; give best= for a {type(model).__name__}")
        best = _incumbent(model, int(latent), bool(minimize))
    return model, acq.desc(minimize, best)


def _incumbent(model, latent: int, minimize: bool) -> float:
    """the max (min with minimize) of the predict_f mean at the model's training inputs"""
    import torch

    L = capi.lib()
    Xd = model._upload(model.X, 1)
    h = model._ensure_handle(max(model._max_batch, 1))
    mu = torch.empty(model.n_latent, Xd.shape[0], dtype=torch.float64, device=model._dev())
    model._chk(L.agp_svgp_predict_f(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), Xd.shape[0], C.c_void_p(mu.data_ptr()), None))
    model._chk(L.agp_ctx_sync(model._ctx))
    return float(mu[latent].min() if minimize else mu[latent].max())


def _check_pending(who: str, pending, pending_noise, D: int, q: int):
    """(n_pending, tau2): the argument checks of the pending points, on the host; pending is None or (n, D)"""
    if not (isinstance(pending_noise, (int, float, np.floating, np.integer)) and math.isfinite(pending_noise) and pending_noise >= 0.0):
        raise ValueError(f"{who}: pending_noise must be finite and >= 0 (got {pending_noise})")
    n = 0
    if pending is not None:
        shape = tuple(pending.shape) if hasattr(pending, "shape") else np.shape(pending)
        if len(shape) != 2 or shape[1] != D:
            raise ValueError(f"{who}: pending must be (n, {D}) (got {tuple(shape)})")
        n = int(shape[0])
    if n + q > capi.ACQ_MAX_PENDING:
        raise ValueError(f"{who}: the pending points and the batch together must not exceed {capi.ACQ_MAX_PENDING} (got {n} + {q})")
    return n, float(pending_noise)


def acquisition(model, acq, X, *, grad: bool = False, latent: int = 0, minimize: bool = False, obsdim: int = 1, pending=None,
                pending_noise: float = 0.0):
    """alpha(x_i) of one latent at the rows of X: (n_t,), and with grad=True (alpha, G) with G[i, d] = d alpha / d x_id, (n_t, D).
    Streamed in chunks of 4096 points, deterministic, the model's state is left as it was (agp_svgp_acquisition).  NumPy in gives
    NumPy out; a torch tensor on the device gives device tensors.  SVGP (AnalyticVI / SVI, QuadratureVI, MCIntegrationVI), VGP, GP,
    OnlineSVGP in Float64; everything else raises NotImplementedError before the device is touched.
    pending=(n, D): the points that are being evaluated already.  The posterior is conditioned on them at their own predicted mean
    with the noise variance pending_noise: mu stays, var shrinks (agp_svgp_acquisition_pending).  pending=None is the call above."""
    if not isinstance(grad, bool):
        raise TypeError("acquisition: grad is a bool")
    if obsdim not in (1, 2):
        raise ValueError("acquisition: obsdim is 1 (points are rows) or 2 (points are columns)")
    model, d = _resolve(model, acq, latent, minimize)
    if pending is not None:
        return _acquisition_pending(model, d, X, grad, int(latent), obsdim, pending, pending_noise)
    import torch

    on_device = isinstance(X, torch.Tensor) and X.is_cuda
    L = capi.lib()
    Xd = model._upload(X, obsdim)
    nt, D = Xd.shape
    h = model._ensure_handle(max(model._max_batch, 1))
    dev = model._dev()
    a = torch.empty(nt, dtype=torch.float64, device=dev)
    G = torch.empty(nt, D, dtype=torch.float64, device=dev) if grad else None
    model._chk(L.agp_svgp_acquisition(h, int(latent), C.byref(d), C.c_void_p(Xd.data_ptr()), Xd.stride(0) if nt else D, nt,
                                      C.c_void_p(a.data_ptr()), C.c_void_p(G.data_ptr()) if grad else None, D))
    model._chk(L.agp_ctx_sync(model._ctx))
    out = (a, G) if grad else (a,)
    if not on_device:
        out = tuple(t.cpu().numpy() for t in out)
    return out if grad else out[0]


def _acquisition_pending(model, d, X, grad, latent, obsdim, pending, pending_noise):
    n, tau2 = _check_pending("acquisition", pending, pending_noise, model.D, 1)
    import torch

    on_device = isinstance(X, torch.Tensor) and X.is_cuda
    L = capi.lib()
    Xd = model._upload(X, obsdim)
    nt, D = Xd.shape
    dev = model._dev()
    Pd = torch.as_tensor(pending, dtype=torch.float64).to(dev).reshape(n, D).contiguous()
    h = model._ensure_handle(max(model._max_batch, 1))
    a = torch.empty(nt, dtype=torch.float64, device=dev)
    G = torch.empty(nt, D, dtype=torch.float64, device=dev) if grad else None
    model._chk(L.agp_svgp_acquisition_pending(h, latent, C.byref(d), C.c_void_p(Pd.data_ptr()) if n else None, D, n, tau2,
                                              C.c_void_p(Xd.data_ptr()), Xd.stride(0) if nt else D, nt, C.c_void_p(a.data_ptr()),
                                              C.c_void_p(G.data_ptr()) if grad else None, D))
    model._chk(L.agp_ctx_sync(model._ctx))
    model._chk(L.agp_svgp_check_status(h))
    out = (a, G) if grad else (a,)
    if not on_device:
        out = tuple(t.cpu().numpy() for t in out)
    return out if grad else out[0]


def acquisition_moments(acq, mu, var, *, minimize: bool = False, grad: bool = False, device: Optional[int] = None):
    """the point function alone on given moments (agp_acq_moments): alpha, and with grad=True (alpha, d alpha / d mu, d alpha / d var)
    with d alpha / d var = d alpha / d sigma / (2 sigma).  var <= 0 takes the defined limit, a NaN moment gives NaN.  best is
    required for EI / PI / LogEI / LogPI.  NumPy in gives NumPy out; device tensors in give device tensors out."""
    if not isinstance(acq, _Acquisition):
        raise TypeError("acq must be UCB(...), EI(...), PI(...), LogEI(...) or LogPI(...)")
    acq.check()
    if acq.kind != ACQ_UCB and acq.best is None:
        raise ValueError(f"{type(acq).__name__}: best must be given (there is no model to take an incumbent from)")
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: augmentedgaussianprocesses.jl_amd has no CPU fallback")
    on_device = isinstance(mu, torch.Tensor) and mu.is_cuda
    dev = mu.device if on_device else torch.device("cuda", device if device is not None else torch.cuda.current_device())
    mud = torch.as_tensor(mu, dtype=torch.float64).to(dev).contiguous()
    vard = torch.as_tensor(var, dtype=torch.float64).to(dev).contiguous()
    if mud.shape != vard.shape:
        raise ValueError("mu and var must have the same shape")
    L = capi.lib()
    ctx = C.c_void_p()
    st = L.agp_ctx_create(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(ctx))
    if st != capi.AGP_OK:
        raise capi.AGPError(st, "agp_ctx_create failed")
    try:
        d = acq.desc(minimize)
        outs = [torch.empty_like(mud) for _ in range(3 if grad else 1)]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        capi.check(ctx, L.agp_acq_moments(ctx, C.byref(d), mud.numel(), ptr(mud), ptr(vard), ptr(outs[0]),
                                          ptr(outs[1]) if grad else None, ptr(outs[2]) if grad else None))
        capi.check(ctx, L.agp_ctx_sync(ctx))
    finally:
        L.agp_ctx_destroy(ctx)
    if not on_device:
        outs = [t.cpu().numpy() for t in outs]
    return tuple(outs) if grad else outs[0]


def maximize_acquisition(model, acq, X0, bounds, *, steps: int = 100, lr=None, beta1: float = 0.9, beta2: float = 0.999,
                         eps: float = 1e-8, latent: int = 0, minimize: bool = False, full: bool = False):
    """multi-start ADAM ascent of the acquisition function inside the box, on the device without a host synchronisation between
    steps (agp_svgp_acq_maximize).  X0 is (R, D); bounds = (lo, hi), each a scalar or of length D; lr a scalar, a vector of length D,
    or None for the interface default 0.02 (hi - lo) per dimension, as in paths.maximize.  Every start climbs for `steps` steps;
    returned is the FINAL iterate of the best start, (x_best (D,), a_best), and with full=True (x_best, a_best, idx, X (R, D), A
    (R,)).  minimize=True is the direction of the OBJECTIVE (UCB becomes the negated lower bound, EI / PI improve downwards); the
    acquisition value is always maximised.  NumPy in gives NumPy out; a device tensor in gives device tensors out.  Every argument
    is checked on the host first."""
    model, d = _resolve(model, acq, latent, minimize)
    shape = tuple(X0.shape) if hasattr(X0, "shape") else np.shape(X0)
    if len(shape) != 2 or shape[1] != model.D:
        raise ValueError(f"X0 must be (R, {model.D}) (got {tuple(shape)})")
    lo, hi, lrv, _, R = check_maximize_args(1, model.D, model.n_latent, shape, bounds, steps, lr, beta1, beta2, eps, latent)
    import torch

    on_device = isinstance(X0, torch.Tensor) and X0.is_cuda
    dev = model._dev()
    D = model.D
    Xd = torch.as_tensor(X0, dtype=torch.float64).to(dev).reshape(R, D).contiguous()
    h = model._ensure_handle(max(model._max_batch, 1))
    X = torch.empty(R, D, dtype=torch.float64, device=dev)
    A = torch.empty(R, dtype=torch.float64, device=dev)
    xb = torch.empty(D, dtype=torch.float64, device=dev)
    ab = torch.empty((), dtype=torch.float64, device=dev)
    ib = torch.empty((), dtype=torch.int64, device=dev)
    as_p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(int(steps), 0, 0, float(beta1), float(beta2), float(eps), as_p(lo), as_p(hi), as_p(lrv))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L = capi.lib()
    model._chk(L.agp_svgp_acq_maximize(h, int(latent), C.byref(d), ptr(Xd), D, R, C.byref(opts), ptr(X) if full else None, D,
                                       ptr(A) if full else None, ptr(xb), ptr(ab), ptr(ib)))
    model._chk(L.agp_ctx_sync(model._ctx))
    out = (xb, ab, ib, X, A) if full else (xb, ab)
    return out if on_device else tuple(t.cpu().numpy() for t in out)


def maximize_acquisition_batch(model, acq, q, X0, bounds, *, pending=None, pending_noise: float = 0.0, steps: int = 100, lr=None,
                               beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, latent: int = 0, minimize: bool = False,
                               full: bool = False):
    """q points for parallel evaluation, picked greedily on the device (agp_svgp_acq_maximize_batch): round b runs the multi-start
    ascent of maximize_acquisition -- the same X0, bounds, steps and best-start rule -- on the acquisition function conditioned on
    `pending` (None or (n, D)) and on the winners of the rounds before, each hallucinated at its own predicted mean with the noise
    variance pending_noise (GP-BUCB / "kriging believer": the mean stays, the variance shrinks, so the next round looks elsewhere).
    n + q <= 64.  Returned is (X_batch (q, D), a_batch (q,)) with a_batch[b] the conditioned acquisition value at X_batch[b], and
    with full=True also idx (q,), the index of each round's winning start.  All rounds are enqueued without a host synchronisation.
    best=None, NumPy or torch inputs and the refused model classes follow maximize_acquisition; every argument is checked on the
    host first."""
    model, d = _resolve(model, acq, latent, minimize)
    if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or q < 1:
        raise ValueError(f"maximize_acquisition_batch: q must be an integer >= 1 (got {q})")
    q = int(q)
    shape = tuple(X0.shape) if hasattr(X0, "shape") else np.shape(X0)
    if len(shape) != 2 or shape[1] != model.D:
        raise ValueError(f"X0 must be (R, {model.D}) (got {tuple(shape)})")
    lo, hi, lrv, _, R = check_maximize_args(1, model.D, model.n_latent, shape, bounds, steps, lr, beta1, beta2, eps, latent)
    n, tau2 = _check_pending("maximize_acquisition_batch", pending, pending_noise, model.D, q)
    import torch

    on_device = isinstance(X0, torch.Tensor) and X0.is_cuda
    dev = model._dev()
    D = model.D
    Xd = torch.as_tensor(X0, dtype=torch.float64).to(dev).reshape(R, D).contiguous()
    Pd = torch.as_tensor(pending, dtype=torch.float64).to(dev).reshape(n, D).contiguous() if n else None
    h = model._ensure_handle(max(model._max_batch, 1))
    xb = torch.empty(q, D, dtype=torch.float64, device=dev)
    ab = torch.empty(q, dtype=torch.float64, device=dev)
    ib = torch.empty(q, dtype=torch.int64, device=dev)
    as_p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(int(steps), 0, 0, float(beta1), float(beta2), float(eps), as_p(lo), as_p(hi), as_p(lrv))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L = capi.lib()
    model._chk(L.agp_svgp_acq_maximize_batch(h, int(latent), C.byref(d), ptr(Pd) if n else None, D, n, tau2, q, ptr(Xd), D, R,
                                             C.byref(opts), ptr(xb), D, ptr(ab), ptr(ib)))
    model._chk(L.agp_ctx_sync(model._ctx))
    model._chk(L.agp_svgp_check_status(h))
    out = (xb, ab, ib) if full else (xb, ab)
    return out if on_device else tuple(t.cpu().numpy() for t in out)


JOINT_STREAM = 3  # the Philox stream of the default base samples: agp_mc_normals(ctx, seed, t=0, stream=3, S, q + n)


def _resolve_joint(who, model, acq, latent, minimize):
    """_resolve, after the kinds that have no joint form are refused by name"""
    if isinstance(acq, _Acquisition) and acq.kind not in (ACQ_UCB, ACQ_EI):
        raise NotImplementedError(f"{who}: {type(acq).__name__} has no joint form here (the joint PI has a zero gradient almost "
                                  f"everywhere, the log kinds need a smoothed maximum): EI(...) or UCB(...)")
    if not isinstance(acq, _Acquisition):
        raise TypeError("acq must be EI(...) or UCB(...)")
    return _resolve(model, acq, latent, minimize)


def _check_joint(who, q, D, pending, samples, seed, base_samples):
    """(n_pending, S): the argument checks of a joint batch, on the host; base_samples is None or (S, q + n)"""
    n = 0
    if pending is not None:
        shape = tuple(pending.shape) if hasattr(pending, "shape") else np.shape(pending)
        if len(shape) != 2 or shape[1] != D:
            raise ValueError(f"{who}: pending must be (n, {D}) (got {tuple(shape)})")
        n = int(shape[0])
    if q < 1:
        raise ValueError(f"{who}: a tuple must hold at least one point (got q = {q})")
    if q + n > capi.ACQ_JOINT_MAX_Q:
        raise ValueError(f"{who}: the batch and the pending points together must not exceed {capi.ACQ_JOINT_MAX_Q} (got {q} + {n})")
    if base_samples is not None:
        shape = tuple(base_samples.shape) if hasattr(base_samples, "shape") else np.shape(base_samples)
        if len(shape) != 2 or shape[1] != q + n:
            raise ValueError(f"{who}: base_samples must be (S, {q + n}) (got {tuple(shape)})")
        S = int(shape[0])
    else:
        if not isinstance(samples, (int, np.integer)) or isinstance(samples, bool):
            raise ValueError(f"{who}: samples must be an integer (got {samples})")
        if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"{who}: seed must be an integer in [0, 2^64) (got {seed})")
        S = int(samples)
    if not 1 <= S <= capi.ACQ_JOINT_MAX_S:
        raise ValueError(f"{who}: the number of samples must lie in [1, {capi.ACQ_JOINT_MAX_S}] (got {S})")
    return n, S


def _base_samples(model, S, K, seed, base_samples):
    """the table (S, K) on the model's device: the caller's, or the draws of (seed, t = 0, stream 3)"""
    import torch

    dev = model._dev()
    if base_samples is not None:
        return torch.as_tensor(base_samples, dtype=torch.float64).to(dev).reshape(S, K).contiguous()
    E = torch.empty(S, K, dtype=torch.float64, device=dev)
    model._chk(capi.lib().agp_mc_normals(model._ctx, int(seed), 0, JOINT_STREAM, S, K, C.c_void_p(E.data_ptr())))
    return E


def acquisition_joint(model, acq, Xq, *, samples: int = 256, seed: int = 0, base_samples=None, grad: bool = False, pending=None,
                      latent: int = 0, minimize: bool = False):
    """The joint Monte-Carlo criterion of tuples of q points (agp_svgp_acquisition_joint): q-EI for EI(...), q-UCB for UCB(...).  Xq is
    (n, q, D) or (q, D); returned is alpha (n,) or a scalar, and with grad=True also the sub-gradient through each sample's winning
    member, (n, q, D) or (q, D).  f_s = mu + L eps_s with L the Cholesky factor of the posterior covariance of the q points and of
    `pending` (None or (n_p, D): members of the joint sample that stay where they are, BoTorch's X_pending -- not hallucinated
    observations); q + n_p <= 16.  The base samples are `base_samples` (S, q + n_p), or the table of agp_mc_normals(seed, t=0,
    stream=3, samples, q + n_p); 1 <= S <= 4096.  PI, LogEI and LogPI have no joint form here and raise NotImplementedError, as the
    model classes that `acquisition` refuses do.  Every argument is checked on the host first."""
    who = "acquisition_joint"
    if not isinstance(grad, bool):
        raise TypeError(f"{who}: grad is a bool")
    model, d = _resolve_joint(who, model, acq, latent, minimize)
    shape = tuple(Xq.shape) if hasattr(Xq, "shape") else np.shape(Xq)
    single = len(shape) == 2
    if single:
        shape = (1,) + shape
    if len(shape) != 3 or shape[2] != model.D:
        raise ValueError(f"{who}: Xq must be (n, q, {model.D}) or (q, {model.D}) (got {tuple(shape)})")
    nsets, q, D = (int(v) for v in shape)
    n, S = _check_joint(who, q, D, pending, samples, seed, base_samples)
    import torch

    on_device = isinstance(Xq, torch.Tensor) and Xq.is_cuda
    dev = model._dev()
    Xd = torch.as_tensor(Xq, dtype=torch.float64).to(dev).reshape(nsets * q, D).contiguous()
    Pd = torch.as_tensor(pending, dtype=torch.float64).to(dev).reshape(n, D).contiguous() if n else None
    h = model._ensure_handle(max(model._max_batch, 1))
    E = _base_samples(model, S, q + n, seed, base_samples)
    a = torch.empty(nsets, dtype=torch.float64, device=dev)
    G = torch.empty(nsets * q, D, dtype=torch.float64, device=dev) if grad else None
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L = capi.lib()
    model._chk(L.agp_svgp_acquisition_joint(h, int(latent), C.byref(d), ptr(Pd) if n else None, D, n, q, ptr(Xd), D, nsets, ptr(E), q + n,
                                            S, ptr(a), ptr(G) if grad else None, D))
    model._chk(L.agp_ctx_sync(model._ctx))
    model._chk(L.agp_svgp_check_status(h))
    a = a[0] if single else a
    if grad:
        G = G.reshape(q, D) if single else G.reshape(nsets, q, D)
    out = (a, G) if grad else (a,)
    if not on_device:
        out = tuple(t.cpu().numpy() for t in out)
    return out if grad else out[0]


def maximize_acquisition_joint(model, acq, X0, bounds, *, samples: int = 256, seed: int = 0, base_samples=None, pending=None,
                               steps: int = 100, lr=None, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, latent: int = 0,
                               minimize: bool = False, full: bool = False):
    """multi-start ADAM ascent of the joint criterion of acquisition_joint over all q points of a tuple together, on the device
    without a host synchronisation between steps (agp_svgp_acq_maximize_joint).  X0 is (R, q, D): a start is a q-tuple (the rows of a
    greedy batch of maximize_acquisition_batch are a natural one); bounds, steps, lr, the recurrence, the clipping and the best-start
    rule are those of maximize_acquisition, per coordinate.  The same base samples serve every start and every step.  Returned is the
    FINAL tuple of the best start, (X_best (q, D), a_best), and with full=True (X_best, a_best, idx, X (R, q, D), A (R,)).  `pending`
    members stay where they are and are not returned.  Every argument is checked on the host first."""
    who = "maximize_acquisition_joint"
    model, d = _resolve_joint(who, model, acq, latent, minimize)
    shape = tuple(X0.shape) if hasattr(X0, "shape") else np.shape(X0)
    if len(shape) != 3 or shape[2] != model.D:
        raise ValueError(f"{who}: X0 must be (R, q, {model.D}) (got {tuple(shape)})")
    R, q, D = (int(v) for v in shape)
    n, S = _check_joint(who, q, D, pending, samples, seed, base_samples)
    lo, hi, lrv, _, _ = check_maximize_args(1, D, model.n_latent, (max(R, 0) * q, D), bounds, steps, lr, beta1, beta2, eps, latent)
    import torch

    on_device = isinstance(X0, torch.Tensor) and X0.is_cuda
    dev = model._dev()
    Xd = torch.as_tensor(X0, dtype=torch.float64).to(dev).reshape(R * q, D).contiguous()
    Pd = torch.as_tensor(pending, dtype=torch.float64).to(dev).reshape(n, D).contiguous() if n else None
    h = model._ensure_handle(max(model._max_batch, 1))
    E = _base_samples(model, S, q + n, seed, base_samples)
    X = torch.empty(R * q, D, dtype=torch.float64, device=dev)
    A = torch.empty(R, dtype=torch.float64, device=dev)
    xb = torch.empty(q, D, dtype=torch.float64, device=dev)
    ab = torch.empty((), dtype=torch.float64, device=dev)
    ib = torch.empty((), dtype=torch.int64, device=dev)
    as_p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(int(steps), 0, 0, float(beta1), float(beta2), float(eps), as_p(lo), as_p(hi), as_p(lrv))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L = capi.lib()
    model._chk(L.agp_svgp_acq_maximize_joint(h, int(latent), C.byref(d), ptr(Pd) if n else None, D, n, q, ptr(Xd), D, R, ptr(E), q + n, S,
                                             C.byref(opts), ptr(X) if full else None, D, ptr(A) if full else None, ptr(xb), D, ptr(ab),
                                             ptr(ib)))
    model._chk(L.agp_ctx_sync(model._ctx))
    model._chk(L.agp_svgp_check_status(h))
    out = (xb, ab, ib, X.reshape(R, q, D), A) if full else (xb, ab)
    return out if on_device else tuple(t.cpu().numpy() for t in out)


def predictor(model, latent: int = 0):
    """(a (m,), A (m, m)): the two objects of the predictor after it has been brought up to date (AGP_VEC_APRED / AGP_MAT_APRED of
    agp_svgp_get_matrix), a = K^-1 mu and A = K^-1 - K^-1 Sigma K^-1 (GP: alpha and Sigma_y^-1), as NumPy arrays.  mu(x) = k*' a and
    var(x) = k** + jitter - k*' A k*; the device forms W = K*m A' (W_ij = sum_l k*_il A[j][l])."""
    import torch

    from .online import OnlineSVGP

    if isinstance(model, OnlineSVGP):
        if model._cur is None:
            raise RuntimeError("the online model has seen no data yet")
        model = model._cur
    if not 0 <= int(latent) < model.n_latent:
        raise ValueError(f"latent must lie in [0, {model.n_latent}) (got {latent})")
    L = capi.lib()
    h = model._ensure_handle(max(model._max_batch, 1))
    dev, m = model._dev(), model.m
    a = torch.empty(m, dtype=model.tdtype, device=dev)
    A = torch.empty(m, m, dtype=model.tdtype, device=dev)
    model._chk(L.agp_svgp_get_matrix(h, int(latent), capi.VEC_APRED, C.c_void_p(a.data_ptr()), 1, m))
    model._chk(L.agp_svgp_get_matrix(h, int(latent), capi.MAT_APRED, C.c_void_p(A.data_ptr()), m, m))
    model._chk(L.agp_ctx_sync(model._ctx))
    return a.cpu().numpy(), A.cpu().numpy()
