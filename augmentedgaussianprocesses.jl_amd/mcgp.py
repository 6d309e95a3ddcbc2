"""MCGP -- the full GP sampled by Gibbs sweeps of the augmented model (src/models/MCGP.jl, src/inference/gibbssampling.jl,
src/training/sampling.jl, src/training/predictions.jl:94-130,260-276).

The device handle is an agp_svgp handle created with AGP_FLAG_FULL | AGP_FLAG_SAMPLED (m = max_batch = N, Z = the training
inputs).  Its state is the current sample f and the sweep counter; `sample` enqueues a whole chain (agp_svgp_gibbs_sample) and keeps
the samples in `model.inference.sample_store`, which the predictors read (agp_svgp_predict_samples).  Every draw is a function of
(seed, sweep, point): include/agp_hip.h, "random streams".
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import capi
from .likelihoods import GaussianLikelihood, LogisticLikelihood, NegBinomialLikelihood, StudentTLikelihood
from .svgp import ELBO, SVGP, _gauss_hermite, objective, predict_f, predict_y, proba_y, refuse_numerical, train_
from .vgp import full_model_args


class GibbsSampling:
    """GibbsSampling(; nBurnin=100, thinning=1, eps=1e-5)  gibbssampling.jl:1-40: draw samples from the true posterior.

    nBurnin: sweeps discarded before samples are kept; thinning: every thinning-th sweep is kept."""

    stoch = False
    batchsize = 0
    optimiser = None
    rho = 1.0

    def __init__(self, nBurnin: int = 100, thinning: int = 1, eps: float = 1e-5):
        if nBurnin < 0:
            raise ValueError("nBurnin should be positive")  # gibbssampling.jl:21
        if thinning < 0:
            raise ValueError("thinning should be positive")  # gibbssampling.jl:22
        self.nBurnin, self.thinning, self.eps = int(nBurnin), int(thinning), float(eps)
        self.n_iter = 0
        self.sample_store = None  # (n, N) array of the kept samples

    def __repr__(self):
        return "Gibbs Sampler"


def kept_sweeps(n: int, discard_initial: int, thinning: int):
    """The sweeps `sample` keeps, 1-based within the call: discard_initial + 1 + k * thinning, k = 0 .. n - 1 (the AbstractMCMC
    convention; agp_svgp_gibbs_sample states it).  The call runs kept_sweeps(...)[-1] sweeps."""
    if n < 1:
        raise ValueError("sample(model, n): n must be at least 1")
    if discard_initial < 0:
        raise ValueError("discard_initial must not be negative")
    if thinning < 1:
        raise ValueError("thinning must be at least 1")
    return [discard_initial + 1 + k * thinning for k in range(n)]


_SAMPLED = (LogisticLikelihood, StudentTLikelihood, NegBinomialLikelihood)


class MCGP(SVGP):
    """MCGP(X, y, kernel, likelihood, GibbsSampling(); verbose=0, optimiser=ADAM(0.01), atfrequency=1, mean=ZeroMean(), obsdim=1).

    Likelihoods: Logistic, StudentT, NegBinomial (r an integer).  `optimiser` and `atfrequency` are kept as the reference keeps
    them: it never tunes an MCGP's kernel.  Float64 only.  `seed` seeds NumPy's generator, from which `sample` takes its seeds."""

    _inference_type = GibbsSampling

    def __init__(self, X, y, kernel, likelihood, inference, *, verbose: int = 0, optimiser=None, atfrequency: int = 1, mean=None,
                 obsdim: int = 1, T=np.float64, device: Optional[int] = None, seed: Optional[int] = None):
        refuse_numerical("MCGP", inference)
        if not isinstance(inference, GibbsSampling):  # MCGP.jl:51-53 (HMCSampling does not exist on this path)
            raise TypeError("The inference object should be of type `SamplingInference` : either `GibbsSampling` or `HMCSampling`")
        if isinstance(likelihood, GaussianLikelihood):  # MCGP.jl:54-56
            raise ValueError("For a Gaussian Likelihood you should directly use the `GP` model or the `SVGP` model for "
                             "large datasets")
        if not isinstance(likelihood, _SAMPLED):  # MCGP.jl:57-58
            raise RuntimeError(f"The {likelihood} is not compatible or implemented with the {inference}")
        if isinstance(likelihood, NegBinomialLikelihood) and float(likelihood.r) != math.floor(float(likelihood.r)):
            raise ValueError("InexactError: the Gibbs sampler of NegBinomialLikelihood(r) draws PolyaGamma(y + Int(r), |f|): "
                             "r must be an integer")  # negativebinomial.jl:87
        X, optimiser = full_model_args("MCGP", "SVGP", inference, X, obsdim, optimiser, mean, T)
        self._desc_flags = capi.FLAG_FULL | capi.FLAG_SAMPLED
        super().__init__(kernel, likelihood, inference, X, verbose=verbose, optimiser=optimiser, atfrequency=atfrequency,
                         mean=mean, Zoptimiser=False, T=T, device=device, seed=seed)
        self.X = X
        yt = self._treat(y)
        if len(yt) != X.shape[0]:
            raise ValueError(f"There is not the same number of samples in X ({X.shape[0]}) and y ({len(yt)})")
        if isinstance(likelihood, NegBinomialLikelihood):
            yv = np.asarray(yt, dtype=np.float64)
            if not np.all((yv >= 0) & (yv == np.floor(yv))):  # PolyaGamma(y + Int(r), |f|): the device latches it as AGP_ERR_LABELS
                raise ValueError("NegBinomialLikelihood: the targets of a Gibbs-sampled model must be non-negative integers")
        self.y = y
        self.N = X.shape[0]
        self.seed = None  # the seed of the chain (set by the first `sample`)
        self.optimiser, self.k_opt = self.k_opt, None  # kept for the record, as the reference keeps it; nothing steps the kernel

    def _ensure_handle(self, max_batch: int = 0):
        return super()._ensure_handle(self.N)  # the full model's handle always holds the whole training set

    def _post_create(self, h):
        pass  # (no hyper-parameter optimiser on the device: the kernel of an MCGP is never tuned)

    def _pull_hypers(self):
        pass

    # ---- the chain ----------------------------------------------------------------------------------------------------------
    def sweep_counter(self) -> int:
        t = C.c_int64()
        self._chk(capi.lib().agp_svgp_gibbs_counter(self._ensure_handle(), 0, C.byref(t)))
        return int(t.value)

    def set_sweep_counter(self, t: int) -> None:
        self._chk(capi.lib().agp_svgp_gibbs_counter(self._ensure_handle(), 1, C.byref(C.c_int64(int(t)))))

    def get_state(self, latent: int = 0):
        """(f, Sigma): the current sample and the conditional covariance of the last sweep (I before the first)"""
        import torch

        dev = self._dev()
        h = self._ensure_handle()
        f = torch.empty(self.N, dtype=self.tdtype, device=dev)
        Sig = torch.empty(self.N, self.N, dtype=self.tdtype, device=dev)
        self._chk(capi.lib().agp_svgp_get_state(h, latent, C.c_void_p(f.data_ptr()), C.c_void_p(Sig.data_ptr()), None, None))
        self._chk(capi.lib().agp_ctx_sync(self._ctx))
        return f.cpu().numpy(), Sig.cpu().numpy()

    def set_f(self, f) -> None:
        """install the sample the chain continues from (load_trained_model)"""
        import torch

        ft = torch.as_tensor(np.asarray(f, dtype=np.float64), dtype=self.tdtype, device=self._dev()).contiguous()
        if ft.numel() != self.N:
            raise ValueError("f needs one value per training point")
        self._chk(capi.lib().agp_svgp_set_state(self._ensure_handle(), 0, C.c_void_p(ft.data_ptr()), None))
        self._chk(capi.lib().agp_ctx_sync(self._ctx))

    def _store_dev(self):
        import torch

        S = self.inference.sample_store
        if S is None or len(S) == 0:
            raise RuntimeError("the model holds no samples yet: call sample(model, n) first")
        return torch.as_tensor(S, dtype=self.tdtype, device=self._dev()).contiguous()

    def _predict_samples(self, X_test, mode: int, obsdim: int = 1):
        import torch

        Xd = self._upload(X_test, obsdim)
        nt = Xd.shape[0]
        St = self._store_dev()
        dev = self._dev()
        o0 = torch.empty(nt, dtype=self.tdtype, device=dev)
        o1 = torch.empty(nt, dtype=self.tdtype, device=dev) if mode != 0 else None
        self._chk(capi.lib().agp_svgp_predict_samples(self._ensure_handle(), C.c_void_p(Xd.data_ptr()), Xd.stride(0), nt,
                                                      C.c_void_p(St.data_ptr()), St.stride(0), St.shape[0], mode,
                                                      C.c_void_p(o0.data_ptr()), C.c_void_p(o1.data_ptr()) if o1 is not None else None))
        self._chk(capi.lib().agp_ctx_sync(self._ctx))
        return o0.cpu().numpy(), (o1.cpu().numpy() if o1 is not None else None)

    def __repr__(self):
        return f"Monte Carlo Gaussian Process with a {self.likelihood} sampled via {self.inference} "  # MCGP.jl:82-87


def sample(model: MCGP, n: int, *, thinning: Optional[int] = None, discard_initial: Optional[int] = None, cat: bool = True,
           seed: Optional[int] = None):
    """sample(model, n; thinning, discard_initial, cat=true)  sampling.jl:11-30: n kept samples as an (n, N) array.

    thinning / discard_initial default to the sampler's thinning / nBurnin.  The samples are kept in
    model.inference.sample_store: appended under cat=True, replacing it otherwise.  seed=None continues with the model's seed, or
    takes a fresh one from the model's NumPy generator when it has none; the seed in use is model.seed.  The sweep counter lives in
    the handle, so with one seed successive calls continue one chain."""
    import torch

    inf = model.inference
    thinning = inf.thinning if thinning is None else int(thinning)
    discard_initial = inf.nBurnin if discard_initial is None else int(discard_initial)
    total = kept_sweeps(n, discard_initial, thinning)[-1]
    if seed is not None:
        model.seed = int(seed)
    elif model.seed is None:
        model.seed = int(model.rng.integers(0, 2 ** 63))
    if not 0 <= model.seed < 2 ** 64:
        raise ValueError("seed must fit 64 bits")
    h = model._ensure_handle()
    if model._data is None:
        model._data = (model._upload(model.X, 1), model._upload_y(model._treat(model.y)), model.N)
    yd = model._data[1]
    store = torch.empty(n, model.N, dtype=model.tdtype, device=model._dev())
    L = capi.lib()
    model._chk(L.agp_svgp_gibbs_sample(h, C.c_void_p(yd.data_ptr()), n, discard_initial, thinning, C.c_uint64(model.seed),
                                       C.c_void_p(store.data_ptr()), store.stride(0)))
    model._chk(L.agp_svgp_check_status(h))  # synchronises: a failed factorisation, a sampler's loop bound
    out = store.cpu().numpy()
    inf.n_iter += total
    if cat and inf.sample_store is not None and len(inf.sample_store):
        inf.sample_store = np.concatenate([inf.sample_store, out], axis=0)
    else:
        inf.sample_store = out.copy()
    model.trained = True
    return out


def sample_local(likelihood, y, f, seed: int, t: int = 0, *, device: Optional[int] = None):
    """sample_local! on given f outside any model (agp_sample_local): (theta, aux) for the Logistic (theta ~ PG(1, |f|)),
    NegBinomial (PG(y + r, |f|)) and StudentT (aux = omega ~ InverseGamma, theta = 1 / omega) likelihoods.  Draw i is a function
    of (seed, t, i) alone."""
    import torch

    L = capi.lib()
    dev = torch.device("cuda", device if device is not None else torch.cuda.current_device())
    ft = torch.as_tensor(np.asarray(f, dtype=np.float64), device=dev).contiguous()
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64), device=dev).contiguous()
    if ft.shape != yt.shape or ft.ndim != 1:
        raise ValueError("y and f are vectors of one length")
    ctx = C.c_void_p()
    st = L.agp_ctx_create(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(ctx))
    if st != capi.AGP_OK:
        raise capi.AGPError(st, "agp_ctx_create failed")
    try:
        th, ax = torch.empty_like(ft), torch.empty_like(ft)
        d = likelihood.lik_desc()
        capi.check(ctx, L.agp_sample_local(ctx, C.byref(d), C.c_void_p(yt.data_ptr()), C.c_void_p(ft.data_ptr()), ft.numel(),
                                           C.c_uint64(int(seed)), int(t), C.c_void_p(th.data_ptr()), C.c_void_p(ax.data_ptr())))
        return th.cpu().numpy(), ax.cpu().numpy()
    finally:
        L.agp_ctx_destroy(ctx)


# ---- prediction (predictions.jl:94-130, 260-276): the MCGP methods of predict_f / predict_y / proba_y ---------------------------
@predict_f.register(MCGP)
def mc_predict_f(model: MCGP, X_test, state=None, *, cov: bool = False, diag: bool = True, obsdim: int = 1):
    if cov and not diag:
        raise NotImplementedError("MCGP: predict_f(...; cov=true, diag=false) needs the n_t x n_t covariance over the samples, "
                                  "which is not formed on the device")
    mu, var = model._predict_samples(X_test, 1 if cov else 0, obsdim)
    return (mu, var) if cov else mu


@predict_y.register(MCGP)
def mc_predict_y(model: MCGP, X_test, state=None, *, obsdim: int = 1):
    """predict_y on the mean of f* over the samples: sign (Bernoulli), the mean (StudentT), r (1 - p) / p with p = logistic(-mu)
    (NegBinomial: predictions.jl:211)"""
    mu, _ = model._predict_samples(X_test, 0, obsdim)
    lik = model.likelihood
    if isinstance(lik, LogisticLikelihood):
        return mu > 0
    if isinstance(lik, NegBinomialLikelihood):
        p = 1.0 / (1.0 + np.exp(mu))
        return lik.r * (1.0 - p) / p
    return mu


@proba_y.register(MCGP)
def mc_proba_y(model: MCGP, X_test, state=None, *, obsdim: int = 1):
    """proba_y(::MCGP) (predictions.jl:260-276): mean and variance over the samples of logistic(f*) for the Bernoulli likelihood.
    Beyond the reference, which defines it for that likelihood only: StudentT / NegBinomial return the two-argument compute_proba of
    the likelihood on the predict_f moments (studentt.jl:57-61; Gauss-Hermite as predictions.jl:225-247)."""
    lik = model.likelihood
    if isinstance(lik, LogisticLikelihood):
        return model._predict_samples(X_test, 2, obsdim)
    mu, var = model._predict_samples(X_test, 1, obsdim)
    if isinstance(lik, StudentTLikelihood):
        return mu, np.maximum(var, 0.0) + lik.nu * lik.sigma ** 2 / (lik.nu - 2.0)
    nodes, weights = _gauss_hermite()
    x = nodes[None, :] * np.sqrt(np.maximum(var, 0.0))[:, None] + mu[:, None]
    sg = 1.0 / (1.0 + np.exp(-x))
    v = sg * lik.r / (1.0 - sg)
    s1 = v @ weights
    return s1, (v * v) @ weights - s1 * s1


@train_.register(MCGP)
def _train_mcgp(model: MCGP, *args, **kwargs):
    raise TypeError("an MCGP is not trained: draw from its posterior with sample(model, n) "
                    "(GibbsSampling has no objective to optimise, MCGP.jl:91)")


@objective.register(MCGP)
@ELBO.register(MCGP)
def _objective_mcgp(model: MCGP, *args, **kwargs) -> float:
    return float("nan")  # objective(::MCGP) = NaN (MCGP.jl:91), and with it ELBO(model)
