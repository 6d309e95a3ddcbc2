"""MOVGP -- the multi-output full variational GP with AnalyticVI (src/models/MOVGP.jl:46-126).

num_latent full latent GPs on the training inputs (kappa = I), mixed by the weights A into one output per task, every task with a
likelihood of its own.  The device handle is an agp_svgp handle created with AGP_FLAG_FULL and the multi-output likelihood (m =
max_batch = N, Z = the training inputs for every latent): the posterior side of a step is VGP's, the likelihood side MOSVGP's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import capi
from .svgp import ELBO, MOSVGP, SVGP, refuse_numerical, train_
from .vgp import VGP, _elbo_vgp, _train_vgp, full_model_args


class MOVGP(MOSVGP):
    """MOVGP(X, y, kernel, likelihoods, inference, num_latent; verbose=0, optimiser=ADAM(0.01), atfrequency=1, mean=ZeroMean(),
    Aoptimiser=ADAM(0.01), obsdim=1).

    X: (N, D) array (rows = points; obsdim=2 takes the transposed layout).  y: one target vector per task.  kernel: one kernel, or
    num_latent of them.  `A=` (n_task, num_latent; rows are used as given) and `seed=` (the draw of A) are this mirror's, as on
    MOSVGP.  Like MOSVGP any num_latent is accepted, not only num_latent == n_task (Appendix A Q7).  Float64 only.
    """

    def __init__(self, X, y, kernel, likelihoods, inference, num_latent: int, *, verbose: int = 0, optimiser=None,
                 atfrequency: int = 1, mean=None, Aoptimiser=None, A=None, obsdim: int = 1, T=np.float64,
                 device: Optional[int] = None, seed: Optional[int] = None):
        Q = int(num_latent)
        if Q < 1:
            raise ValueError("num_latent must be positive")
        if isinstance(kernel, (list, tuple)) and len(kernel) != Q:  # MOVGP.jl:94-95
            raise ValueError("Number of kernels should be equal to the number of tasks")
        refuse_numerical("MOVGP", inference)
        X, optimiser = full_model_args("MOVGP", "MOSVGP", inference, X, obsdim, optimiser, mean, T)
        self._desc_flags = capi.FLAG_FULL
        super().__init__(kernel, likelihoods, inference, [X] * Q, Aoptimiser=Aoptimiser, A=A, verbose=verbose,
                         optimiser=optimiser, atfrequency=atfrequency, mean=mean, Zoptimiser=False, T=T, device=device,
                         seed=seed)
        self.X = X
        yt = self._treat(y)
        if yt.shape[-1] != X.shape[0]:
            raise ValueError(f"There is not the same number of samples in X ({X.shape[0]}) and y ({yt.shape[-1]})")
        self.y = [np.asarray(v) for v in y]
        self.N = X.shape[0]

    def _ensure_handle(self, max_batch: int):
        return SVGP._ensure_handle(self, self.N)  # the full model's handle always holds the whole training set

    hypergrad = VGP.hypergrad  # only the Gaussian KL depends on a latent's kernel; X is not optimised

    def __repr__(self):
        return (f"Multioutput Variational Gaussian Process with the likelihoods {self.likelihood} "
                f"infered by {self.inference} ")


# train!(model::MOVGP, iterations) and ELBO(model): a full model's, on its own training set (vgp.py)
train_.register(MOVGP)(_train_vgp)
ELBO.register(MOVGP)(_elbo_vgp)
