"""VGP -- the full (non-sparse) variational GP with AnalyticVI (src/models/VGP.jl:36-85).

One latent of dimension N per n_latent(likelihood), kappa = I: the device handle is an agp_svgp handle created with
AGP_FLAG_FULL (m = max_batch = N, Z = the training inputs), so every entry point keeps its SVGP meaning with Z = X.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from .likelihoods import GaussianLikelihood
from .svgp import ADAM, ELBO, SVGP, AnalyticVI, QuadratureVI, check_numerical, train_


def full_model_args(name, sparse, inference, X, obsdim, optimiser, mean, T):
    """What the constructors of the full models (VGP, MOVGP) share: the refusals (AnalyticSVI, a float type other than Float64, an
    EmpiricalMean of another length than N), X as a contiguous (N, D) array, and the optimiser default ADAM(0.01) for None / True
    (VGP.jl:63, MOVGP.jl:57; the SVGP constructor maps False to "off").  `sparse`: the model to name for AnalyticSVI.
    Returns (X, optimiser)."""
    if getattr(inference, "stoch", False):
        # the reference constructs the model with AnalyticSVI, but natural_gradient!(::VarLatent) cannot run on a minibatch
        raise ValueError(f"{name} takes the full data set every iteration: use AnalyticVI(), or {sparse} for AnalyticSVI")
    if np.dtype(T) != np.dtype(np.float64):
        raise NotImplementedError(f"{name} runs in Float64 only (the full N x N factorisation has no Float32 path)")
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if obsdim == 2:
        X = X.T
    X = np.ascontiguousarray(X)
    if optimiser is None or optimiser is True:
        optimiser = ADAM(0.01)
    if mean is not None and not np.isscalar(mean) and len(mean) != X.shape[0]:
        raise ValueError("an EmpiricalMean needs one value per training point")
    return X, optimiser


class VGP(SVGP):
    """VGP(X, y, kernel, likelihood, inference; verbose=0, optimiser=ADAM(0.01), atfrequency=1, mean=ZeroMean(), obsdim=1).

    X: (N, D) array (rows = points; obsdim=2 takes the transposed layout).  `optimiser=True` is ADAM(0.01) (VGP.jl:63, unlike
    SVGP's 0.001).  A Real mean gives ConstantMean, a vector EmpiricalMean (VGP.jl:68-72).  Float64 only.

    inference: AnalyticVI(), QuadratureVI(...) (nvi.py) for the Logistic, StudentT and Laplace likelihoods, or MCIntegrationVI(...)
    for the SoftMax and LogisticSoftMax likelihoods (K latents).  With either of the two the handle keeps (mu, Sigma) and the
    optimiser's moments per latent (AGP_FLAG_NUMERICAL), and `optimiser` must be False: the hyper-parameter step through the
    numerical ELBO is not built, and the default ADAM(0.01) is refused rather than silently switched off.
    """

    def __init__(self, X, y, kernel, likelihood, inference, *, verbose: int = 0, optimiser=None, atfrequency: int = 1,
                 mean=None, obsdim: int = 1, T=np.float64, device: Optional[int] = None):
        if not isinstance(inference, (AnalyticVI, QuadratureVI)):  # VGP.jl:51
            raise TypeError("The inference object should be of type `VariationalInference` : either `AnalyticVI` or "
                            "`NumericalVI`")
        self._numerical = isinstance(inference, QuadratureVI)
        if self._numerical:
            check_numerical("VGP", inference, likelihood, optimiser, T)
            if inference.stoch:
                raise ValueError("VGP takes the full data set every iteration: use " +
                                 ("MCIntegrationVI(), or SVGP for MCIntegrationSVI" if getattr(inference, "mc", False)
                                  else "QuadratureVI(), or SVGP for QuadratureSVI"))
        if isinstance(likelihood, GaussianLikelihood):  # VGP.jl:54-56
            raise ValueError("For a Gaussian Likelihood you should directly use the `GP` model or the `SVGP` model for "
                             "large datasets")
        X, optimiser = full_model_args("VGP", "SVGP", inference, X, obsdim, optimiser, mean, T)
        self._desc_flags = capi.FLAG_FULL | (capi.FLAG_NUMERICAL if self._numerical else 0) | (capi.FLAG_MC if getattr(inference, "mc", False) else 0)
        super().__init__(kernel, likelihood, inference, X, verbose=verbose, optimiser=optimiser, atfrequency=atfrequency,
                         mean=mean, Zoptimiser=False, T=T, device=device)
        self.nvi_alphas = []  # QuadratureVI: alpha of every step taken (the backtracking's accepted step length); MCIntegrationVI: a K-tuple
        self.X = X
        yt = self._treat(y)
        if len(yt) != X.shape[0]:
            raise ValueError(f"There is not the same number of samples in X ({X.shape[0]}) and y ({len(yt)})")
        self.y = y
        self.N = X.shape[0]

    def _ensure_handle(self, max_batch: int = 0):
        return super()._ensure_handle(self.N)  # the full model's handle always holds the whole training set

    def hypergrad(self, latent: int = 0):
        """(d variance, d scales[D]) of the ELBO's Gaussian KL after the last step (autotuning.jl:49-85); X is not optimised."""
        dv = C.c_double()
        ds = (C.c_double * self.D)()
        self._chk(capi.lib().agp_svgp_hypergrad(self._h, latent, C.byref(dv), ds, None))
        return dv.value, np.array(list(ds))

    def __repr__(self):
        return (f"Variational Gaussian Process with a {self.likelihood} infered by {self.inference} "
                f"(N = {self.N}, {self.n_latent} latent(s))")


def n_latent(model) -> int:
    """n_latent(model): number of latent GPs"""
    return model.n_latent


@train_.register(VGP)
def _train_vgp(model: VGP, *args, iterations: Optional[int] = None, callback=None, state=None, convergence=None):
    """train!(model::VGP, iterations; callback, state)  (training.jl:113-120): full batch on the model's own data.
    train_(model, iterations) is the reference's form; train_(model, X, y, iterations) is accepted when (X, y) are the model's own
    training set -- the latent of a full model is tied to its data, so other data is refused."""
    if len(args) == 1:
        iterations = args[0]
    elif len(args) in (2, 3):
        X, y = args[0], args[1]
        if len(args) == 3:
            iterations = args[2]
        if not (np.shape(X) == model.X.shape and np.array_equal(np.asarray(X, dtype=np.float64), model.X)
                and np.array_equal(np.asarray(y), np.asarray(model.y))):
            raise ValueError(f"a {type(model).__name__} trains on the data it was built with: train_(model, iterations)")
    elif args:
        raise TypeError("train_(model::VGP, iterations)")
    if iterations is None:
        iterations = 100
    if getattr(model, "_numerical", False):
        if convergence is not None:
            raise NotImplementedError("train_(model::VGP with QuadratureVI): convergence= is not wired")
        from .nvi import train_numerical

        return train_numerical(model, iterations, callback=callback, state=state)  # (X = None: the model's own data)
    return train_.dispatch(SVGP)(model, model.X, model.y, iterations, callback=callback, state=state,
                                 convergence=convergence)


@ELBO.register(VGP)
def _elbo_vgp(model: VGP) -> float:
    """ELBO(model) of a full model: the ELBO on its own training set (ELBO.jl:28-47 with X = the training inputs, rho = 1):
    fresh local variables from the current posterior, one local update, then expectation - GaussianKL - AugmentedKL."""
    L = capi.lib()
    Xd = model._upload(model.X, 1)
    yd = model._upload_y(model._treat(model.y))
    h = model._ensure_handle(model.N)
    out = C.c_double()
    model._chk(L.agp_svgp_elbo(h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), None, model.N, 1.0, 1,
                               C.byref(out)))
    return out.value
