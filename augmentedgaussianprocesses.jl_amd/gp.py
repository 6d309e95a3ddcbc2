"""GP -- exact Gaussian-process regression with Analytic() inference (src/models/GP.jl:37-92, src/inference/analytic.jl).

The device handle is an agp_svgp handle created with AGP_FLAG_FULL | AGP_FLAG_EXACT (m = max_batch = N, Z = the training inputs):
a step factors Sigma = K + sigma2 I, forms alpha = Sigma \\ (y - mu0) and log p, and takes the noise step, all on the device.

elbo_mode="corrected" (default) fixes three defects of the reference; elbo_mode="reference" reproduces them:
G1 the kernel never moves (the reference's gradient is `nothing`), G2 the noise gradient takes ||alpha||_2 where alpha' alpha is
meant, G3 log p uses y where y - mu0 is meant.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import numpy as np

from . import capi
from .likelihoods import GaussianLikelihood
from .svgp import ADAM, ELBO, SVGP, Analytic, train_
from .vgp import VGP


class GP(SVGP):
    """GP(X, y, kernel; noise=1e-5, opt_noise=true, verbose=0, optimiser=ADAM(0.01), atfrequency=1, mean=ZeroMean(), obsdim=1).

    The likelihood is GaussianLikelihood(noise; opt_noise) (opt_noise=True: ADAM(0.05)), the inference Analytic().  A Bool
    `optimiser` gives ADAM(0.01) or no kernel optimisation; a Real mean ConstantMean, a vector EmpiricalMean (never learned).  As in
    the reference the constructor ends with train_(model, 1) (GP.jl:63).  Float64 only.
    """

    def __init__(self, X, y, kernel, *, noise: float = 1e-5, opt_noise=True, verbose: int = 0, optimiser=True, atfrequency: int = 1,
                 mean=None, obsdim: int = 1, elbo_mode: str = "corrected", T=np.float64, device: Optional[int] = None,
                 _initial_train: bool = True):
        if np.dtype(T) != np.dtype(np.float64):
            raise NotImplementedError("GP runs in Float64 only (the full N x N factorisation has no Float32 path)")
        if elbo_mode not in ("corrected", "reference"):
            raise ValueError("elbo_mode is 'corrected' or 'reference'")
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        if obsdim == 2:
            X = X.T
        X = np.ascontiguousarray(X)
        yv = np.asarray(y, dtype=np.float64).reshape(-1)
        if len(yv) != X.shape[0]:
            raise ValueError(f"There is not the same number of samples in X ({X.shape[0]}) and y ({len(yv)})")
        if isinstance(optimiser, bool):
            optimiser = ADAM(0.01) if optimiser else None  # GP.jl:53-55
        if optimiser is None:
            optimiser = False  # (SVGP's constructor maps None to its own default)
        if mean is not None and not np.isscalar(mean) and len(mean) != X.shape[0]:
            raise ValueError("an EmpiricalMean needs one value per training point")
        likelihood = GaussianLikelihood(noise, opt_noise=opt_noise)
        self._desc_flags = capi.FLAG_FULL | capi.FLAG_EXACT
        super().__init__(kernel, likelihood, Analytic(), X, verbose=verbose, optimiser=optimiser, atfrequency=atfrequency,
                         mean=mean, Zoptimiser=False, T=T, device=device, elbo_mode=elbo_mode)
        self.X = X
        self.y = yv
        self.N = X.shape[0]
        self._g1_warned = False
        self._mean_fixed = True  # (mu0 is never learned: no prior-mean step behind the hyper step)
        if _initial_train:
            train_(self, 1)

    def _ensure_handle(self, max_batch: int):
        return super()._ensure_handle(self.N)  # the full model's handle always holds the whole training set

    def hypergrad(self, latent: int = 0):
        """(d log p / d variance, d log p / d scales[D]) at the stored posterior (G1 corrected; zeros in the reference mode)"""
        return VGP.hypergrad(self, latent)

    def get_state(self, latent: int = 0):
        """(alpha, Sigma) of the posterior (GP.jl: Posterior(Sigma, alpha)); there are no natural parameters."""
        torch = _torch()
        dev = self._dev()
        alpha = torch.empty(self.N, dtype=self.tdtype, device=dev)
        Sig = torch.empty(self.N, self.N, dtype=self.tdtype, device=dev)
        self._chk(capi.lib().agp_svgp_get_state(self._h, latent, C.c_void_p(alpha.data_ptr()), C.c_void_p(Sig.data_ptr()), None,
                                                None))
        self._chk(capi.lib().agp_ctx_sync(self._ctx))
        return alpha.cpu().numpy(), Sig.cpu().numpy()

    def _bind(self):
        """the targets on the device of a handle that has taken no step (load_trained_model): post_step! with the current sigma2"""
        Xd = self._upload(self.X, 1)
        yd = self._upload_y(self.y)
        h = self._ensure_handle(self.N)
        out = C.c_double()
        self._chk(capi.lib().agp_svgp_elbo(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), None, self.N, 1.0,
                                           0, C.byref(out)))
        self._data = (Xd, yd, self.N)

    def __repr__(self):
        return f"Gaussian Process with a {self.likelihood} infered by {self.inference} "  # GP.jl:70-73


def _torch():
    import torch

    return torch


@train_.register(GP)
def _train_gp(model: GP, *args, iterations: Optional[int] = None, callback=None, state=None, convergence=None):
    """train!(model::GP, iterations) (training.jl:113-120) on the model's own data; train_(model, X, y, iterations) is accepted when
    (X, y) are that data."""
    if len(args) == 1:
        iterations = args[0]
    elif len(args) in (2, 3):
        X, y = args[0], args[1]
        if len(args) == 3:
            iterations = args[2]
        if not (np.shape(X) == model.X.shape and np.array_equal(np.asarray(X, dtype=np.float64), model.X)
                and np.array_equal(np.asarray(y, dtype=np.float64).reshape(-1), model.y)):
            raise ValueError("a GP trains on the data it was built with: train_(model, iterations)")
    elif args:
        raise TypeError("train_(model::GP, iterations)")
    if iterations is None:
        iterations = 100
    if model.elbo_mode == "reference" and model.k_opt is not None and not model._g1_warned:
        # G1: update_hyperparameters!(::GP) differentiates a function of the stored Sigma and gets `nothing` (autotuning.jl:5-37)
        n0 = model.inference.n_iter
        if any(n % model.atfrequency == 0 and n >= 3 for n in range(n0, n0 + int(iterations) - 1)):
            warnings.warn("Kernel gradients are equal to zero", stacklevel=2)
            model._g1_warned = True
    return train_.dispatch(SVGP)(model, model.X, model.y, iterations, callback=callback, state=state, convergence=convergence)


@ELBO.register(GP)
def _elbo_gp(model: GP, *args, **kwargs) -> float:
    """ELBO(model) of a GP: log p(y) of the stored posterior (GP.jl:87-92)."""
    if model._data is None:
        model._bind()
    Xd, yd, N = model._data
    out = C.c_double()
    model._chk(capi.lib().agp_svgp_elbo(model._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), None, N, 1.0,
                                        0, C.byref(out)))
    return out.value
