"""Pathwise posterior sampling: function draws from a trained SVGP, VGP or GP (include/agp_hip.h, "PATHWISE SAMPLING").

    paths = AGP.sample_paths(model, n_samples, n_features=1024, seed=None, t=0)
    F = paths(X_test)          # (n_samples, n_t), or (n_latent, n_samples, n_t) for several latents
    G = paths.grad(X_test)     # (n_samples, n_t, D): d f_s / d x, in closed form from the draw's tables; value=True gives (F, G)
    x, f = paths.maximize(X0, (lo, hi), steps=100)   # (n_samples, D), (n_samples,): every path's best of R ADAM ascents, on the device

Decoupled sampling (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors"): a prior function from
random Fourier features, a draw u ~ q(u), Matheron's correction.  A draw is an ordinary function: it can be evaluated at any number
of points, streamed, and it is a snapshot -- training the model further, changing its kernel or freeing it does not change the
paths.  Everything random is a function of (seed, t, latent): the same arguments give the same paths bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi

N_MAX = 65536  # n_features and n_samples (agp_svgp_pathwise_draw)
CTR_MAX = 2 ** 32  # products that index one 32-bit counter word, and the draw counter t
GRAD_REFUSAL_EXPONENTIAL = "ExponentialKernel is not differentiable at zero distance"  # agp_pathwise_eval_grad says the same

MAX_D_ASCENT = 64  # agp_pathwise_maximize
MAX_STEPS = 65536


def check_maximize_args(n_samples: int, D: int, n_latent: int, x0_shape, bounds, steps=100, lr=None, beta1=0.9, beta2=0.999,
                        eps=1e-8, latent=0):
    """every argument check of paths.maximize / agp_pathwise_maximize, on the host before any device call.  x0_shape is (R, D) for
    shared starts or (S, R, D) per sample.  Returns (lo, hi, lr, shared, R): the box and the step sizes as float64 arrays of length
    D.  lr=None is the interface default 0.02 (hi - lo) per dimension -- a default, not a tuned value; a dimension pinned by
    lo = hi then gets the step size 1, which the box makes irrelevant."""
    if int(D) > MAX_D_ASCENT:
        raise NotImplementedError(f"paths.maximize: D > {MAX_D_ASCENT} is not supported (D = {D})")
    if not 0 <= int(latent) < int(n_latent):
        raise ValueError(f"latent must lie in [0, {n_latent}) (got {latent})")
    shape = tuple(int(v) for v in x0_shape)
    if len(shape) == 2 and shape[1] == D:
        shared, R = True, shape[0]
    elif len(shape) == 3 and shape[0] == n_samples and shape[2] == D:
        shared, R = False, shape[1]
    else:
        raise ValueError(f"X0 must be (R, {D}) for shared starts or ({n_samples}, R, {D}) per sample (got {shape})")
    if R < 1 or n_samples * R >= 2 ** 31:
        raise ValueError(f"the number of starts must be >= 1 and n_samples * starts below 2^31 (got {R})")
    if not (isinstance(bounds, (tuple, list)) and len(bounds) == 2):
        raise ValueError("bounds must be a pair (lo, hi), each a scalar or of length D")

    def vec(v, name):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(D, float(a))
        if a.shape != (D,):
            raise ValueError(f"{name} must be a scalar or of length {D} (got shape {a.shape})")
        return np.ascontiguousarray(a)

    lo, hi = vec(bounds[0], "lo"), vec(bounds[1], "hi")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("the bounds must be finite")
    if np.any(lo > hi):
        raise ValueError("the bounds must satisfy lo <= hi in every dimension")
    if lr is None:
        lrv = 0.02 * (hi - lo)
        lrv[lrv == 0.0] = 1.0
    else:
        lrv = vec(lr, "lr")
    if not (np.all(np.isfinite(lrv)) and np.all(lrv > 0.0)):
        raise ValueError("the step sizes lr must be finite and > 0")
    if not 0 <= int(steps) <= MAX_STEPS:
        raise ValueError(f"steps must lie in [0, {MAX_STEPS}] (got {steps})")
    for name, b in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= float(b) < 1.0:
            raise ValueError(f"{name} must lie in [0, 1) (got {b})")
    if not (np.isfinite(eps) and float(eps) > 0.0):
        raise ValueError(f"eps must be finite and > 0 (got {eps})")
    return lo, hi, lrv, shared, R


def check_draw_args(m: int, D: int, n_samples: int, n_features: int, t: int, seed: Optional[int] = None) -> None:
    """the argument limits of agp_svgp_pathwise_draw, raised on the host before anything is created"""
    if not 1 <= int(n_samples) <= N_MAX:
        raise ValueError(f"n_samples must lie in [1, {N_MAX}] (got {n_samples})")
    if not 1 <= int(n_features) <= N_MAX:
        raise ValueError(f"n_features must lie in [1, {N_MAX}] (got {n_features})")
    if n_features * D >= CTR_MAX or n_features * n_samples >= CTR_MAX or m * n_samples >= CTR_MAX:
        raise ValueError("n_features * D, n_features * n_samples and m * n_samples must stay below 2^32")
    if not 0 <= int(t) < CTR_MAX:
        raise ValueError("the draw counter t must lie in [0, 2^32)")
    if seed is not None and not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must fit 64 bits")


def refusal(model) -> Optional[str]:
    """why this model has no pathwise draw, by name, or None (the host mirror of the device's AGP_ERR_UNSUPPORTED list)"""
    from .mcgp import MCGP
    from .movgp import MOVGP
    from .svgp import MOSVGP

    if isinstance(model, (MOSVGP, MOVGP)):
        return "multi-output models (MOSVGP, MOVGP) are not supported: draw from single-output models"
    if isinstance(model, MCGP):
        return "an MCGP (GibbsSampling) is not supported: its samples are read by predict_f / proba_y"
    if getattr(model, "_numerical", False):
        return ("numerical inference (QuadratureVI, MCIntegrationVI) is not supported yet -- a follow-up: the factor of Sigma is "
                "already kept on such a handle")
    if np.dtype(model.T) != np.dtype(np.float64):
        return "Float32 models are not supported (the draw is Float64)"
    if getattr(model, "latent_offset", 0) != 0 or getattr(model, "n_latent_total", model.n_latent) != model.n_latent:
        return "latent-sharded models are not supported (a draw needs every latent on one handle)"
    return None


class PathwiseSamples:
    """n_samples function draws from a model's posterior; call it on test inputs.  Owns an agp_pathwise object on the device."""

    def __init__(self, model, n_samples: int, n_features: int, seed: int, t: int):
        self._model = model  # keeps the context alive (the draw uses its stream)
        self.n_samples, self.n_features, self.seed, self.t = int(n_samples), int(n_features), int(seed), int(t)
        self.n_latent, self.m, self.D = model.n_latent, model.m, model.D
        self._kinds = tuple(k._kind for k in model.kernels)  # of the snapshot: what grad refuses is decided on the host
        self._p = None
        h = model._ensure_handle(max(model._max_batch, 1))
        p = C.c_void_p()
        model._chk(capi.lib().agp_svgp_pathwise_draw(h, self.n_features, self.n_samples, C.c_uint64(self.seed), self.t, C.byref(p)))
        self._p = p

    def _live(self):
        if self._p is None:
            raise RuntimeError("the paths have been freed")
        return self._p

    def __call__(self, X_test, *, obsdim: int = 1):
        """the paths at X_test: (n_samples, n_t), or (n_latent, n_samples, n_t) for several latents.  NumPy in gives NumPy out; a
        torch tensor on the device gives a device tensor."""
        import torch

        p, model = self._live(), self._model
        on_device = isinstance(X_test, torch.Tensor) and X_test.is_cuda
        Xd = model._upload(X_test, obsdim)
        nt = Xd.shape[0]
        out = torch.empty(self.n_latent, self.n_samples, nt, dtype=torch.float64, device=model._dev())
        L = capi.lib()
        model._chk(L.agp_pathwise_eval(p, C.c_void_p(Xd.data_ptr()), Xd.stride(0) if nt else self.D, nt, C.c_void_p(out.data_ptr()),
                                       max(nt, 1)))
        model._chk(L.agp_ctx_sync(model._ctx))
        if self.n_latent == 1:
            out = out[0]
        return out if on_device else out.cpu().numpy()

    def grad(self, X_test, *, value: bool = False, obsdim: int = 1):
        """the input gradients of the paths at X_test: G[s, i, d] = d f_s / d x_d (x_i), (n_samples, n_t, D), or (n_latent, n_samples,
        n_t, D) for several latents; value=True returns (F, G) with F exactly what paths(X_test) returns.  Closed form from the
        draw's own tables (agp_pathwise_eval_grad): what maximising a draw by gradient ascent -- Thompson sampling -- needs.  NumPy in
        gives NumPy out; a torch tensor on the device gives device tensors.  A draw with an ExponentialKernel raises
        NotImplementedError before the device is touched."""
        import torch

        p, model = self._live(), self._model
        if capi.K_EXPONENTIAL in self._kinds:
            raise NotImplementedError("paths.grad: " + GRAD_REFUSAL_EXPONENTIAL)
        on_device = isinstance(X_test, torch.Tensor) and X_test.is_cuda
        Xd = model._upload(X_test, obsdim)
        nt = Xd.shape[0]
        dev = model._dev()
        G = torch.empty(self.n_latent, self.n_samples, nt, self.D, dtype=torch.float64, device=dev)
        F = torch.empty(self.n_latent, self.n_samples, nt, dtype=torch.float64, device=dev) if value else None
        L = capi.lib()
        model._chk(L.agp_pathwise_eval_grad(p, C.c_void_p(Xd.data_ptr()), Xd.stride(0) if nt else self.D, nt,
                                            C.c_void_p(F.data_ptr()) if value else None, max(nt, 1), C.c_void_p(G.data_ptr()),
                                            max(nt, 1), self.D))
        model._chk(L.agp_ctx_sync(model._ctx))
        out = [t[0] if self.n_latent == 1 else t for t in ((F, G) if value else (G,))]
        if not on_device:
            out = [t.cpu().numpy() for t in out]
        return tuple(out) if value else out[0]

    def maximize(self, X0, bounds, *, steps: int = 100, lr=None, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 latent: int = 0, minimize: bool = False, full: bool = False):
        """multi-start ADAM ascent of the paths on the device, one launch (agp_pathwise_maximize): Thompson sampling's inner loop.
        X0 is (R, D), the same starts for every path, or (S, R, D); bounds = (lo, hi), each a scalar or of length D; lr a scalar, a
        vector of length D, or None for the interface default 0.02 (hi - lo) per dimension (a default, not a tuned value).  Every
        path s climbs from each of its R starts for `steps` steps inside the box; returned is the FINAL iterate of the best start:
        (x_best (S, D), f_best (S,)), with full=True (x_best, f_best, idx (S,), X (S, R, D), F (S, R)).  minimize=True descends
        and picks the smallest value.  NumPy in gives NumPy out; a torch tensor on the device gives device tensors.  Every
        argument is checked on the host first (check_maximize_args); a latent with an ExponentialKernel raises NotImplementedError
        before the device is touched."""
        p = self._live()
        if not 0 <= int(latent) < self.n_latent:
            raise ValueError(f"latent must lie in [0, {self.n_latent}) (got {latent})")
        if self._kinds[int(latent)] == capi.K_EXPONENTIAL:
            raise NotImplementedError("paths.maximize: " + GRAD_REFUSAL_EXPONENTIAL)
        lo, hi, lrv, shared, R = check_maximize_args(self.n_samples, self.D, self.n_latent, tuple(X0.shape) if hasattr(X0, "shape") else np.shape(X0), bounds, steps, lr, beta1, beta2,
                                                     eps, latent)
        import torch

        model = self._model
        on_device = isinstance(X0, torch.Tensor) and X0.is_cuda
        dev = model._dev()
        Xd = torch.as_tensor(X0, dtype=torch.float64).to(dev).reshape(-1, self.D).contiguous()
        S, D = self.n_samples, self.D
        X = torch.empty(S, R, D, dtype=torch.float64, device=dev)
        F = torch.empty(S, R, dtype=torch.float64, device=dev)
        xb = torch.empty(S, D, dtype=torch.float64, device=dev)
        fb = torch.empty(S, dtype=torch.float64, device=dev)
        ib = torch.empty(S, dtype=torch.int64, device=dev)
        as_p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        opts = capi.PwAscentOpts(int(steps), int(bool(minimize)), int(shared), float(beta1), float(beta2), float(eps), as_p(lo), as_p(hi),
                                 as_p(lrv))
        ptr = lambda t: C.c_void_p(t.data_ptr())
        L = capi.lib()
        model._chk(L.agp_pathwise_maximize(p, int(latent), ptr(Xd), D, R, C.byref(opts), ptr(X) if full else None, D,
                                           ptr(F) if full else None, R, ptr(xb), D, ptr(fb), ptr(ib)))
        model._chk(L.agp_ctx_sync(model._ctx))
        out = (xb, fb, ib, X, F) if full else (xb, fb)
        return out if on_device else tuple(t.cpu().numpy() for t in out)

    def tables(self, latent: int = 0):
        """the draw's tables of one latent as NumPy arrays: omega (l, D), phase (l), W (l, S), V (m, S), E (m, S)"""
        import torch

        p, model = self._live(), self._model
        dev = model._dev()
        shapes = {"omega": (capi.PW_OMEGA, (self.n_features, self.D)), "phase": (capi.PW_PHASE, (self.n_features,)),
                  "W": (capi.PW_W, (self.n_features, self.n_samples)), "V": (capi.PW_V, (self.m, self.n_samples)),
                  "E": (capi.PW_E, (self.m, self.n_samples))}
        out = {}
        for name, (which, shp) in shapes.items():
            buf = torch.empty(*shp, dtype=torch.float64, device=dev)
            model._chk(capi.lib().agp_pathwise_get(p, int(latent), which, C.c_void_p(buf.data_ptr()), shp[-1]))
            out[name] = buf
        model._chk(capi.lib().agp_ctx_sync(model._ctx))
        return {k: v.cpu().numpy() for k, v in out.items()}

    def free(self) -> None:
        """release the device object (idempotent)"""
        if self._p is not None:
            capi.lib().agp_pathwise_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __repr__(self):
        return (f"PathwiseSamples({self.n_samples} paths, {self.n_features} features, {self.n_latent} latent(s), "
                f"seed={self.seed}, t={self.t})")


def sample_paths(model, n_samples: int, *, n_features: int = 1024, seed: Optional[int] = None, t: int = 0) -> PathwiseSamples:
    """sample_paths(model, n_samples; n_features=1024, seed=nothing, t=0): joint function draws from the posterior of an SVGP, VGP
    (AnalyticVI / AnalyticSVI), GP or OnlineSVGP.  seed=None takes the model's seed (drawn once from the model's generator, as
    `sample` does for an MCGP); t is the caller's draw counter: another t, another independent draw from the same seed."""
    from .svgp import SVGP

    if not isinstance(model, SVGP) and hasattr(model, "_cur"):  # OnlineSVGP: the wrapper that owns the current handle
        if model._cur is None:
            raise RuntimeError("the online model has seen no data yet")
        model = model._cur
    if not isinstance(model, SVGP):
        raise TypeError("sample_paths(model, n): model must be an SVGP, VGP, GP or OnlineSVGP")
    why = refusal(model)
    if why is not None:
        raise NotImplementedError("sample_paths: " + why)
    check_draw_args(model.m, model.D, n_samples, n_features, t, seed)
    if seed is None:
        if getattr(model, "seed", None) is None:
            model.seed = int(model.rng.integers(0, 2 ** 63))
        seed = model.seed
    return PathwiseSamples(model, n_samples, n_features, int(seed), t)


def pathwise_features(kernel, D: int, n_features: int, seed: int, t: int = 0, latent: int = 0, *, device: Optional[int] = None):
    """the spectral draw alone, outside any model (agp_pathwise_features): (omega (l, D), phase (l)) as NumPy arrays"""
    import torch

    check_draw_args(1, D, 1, n_features, t, seed)
    L = capi.lib()
    dev = torch.device("cuda", device if device is not None else torch.cuda.current_device())
    ctx = C.c_void_p()
    st = L.agp_ctx_create(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(ctx))
    if st != capi.AGP_OK:
        raise capi.AGPError(st, "agp_ctx_create failed")
    try:
        kd, keep = kernel.desc(D)
        om = torch.empty(n_features, D, dtype=torch.float64, device=dev)
        ph = torch.empty(n_features, dtype=torch.float64, device=dev)
        capi.check(ctx, L.agp_pathwise_features(ctx, C.byref(kd), D, n_features, C.c_uint64(int(seed)), int(t), int(latent),
                                                C.c_void_p(om.data_ptr()), C.c_void_p(ph.data_ptr())))
        return om.cpu().numpy(), ph.cpu().numpy()
    finally:
        L.agp_ctx_destroy(ctx)
