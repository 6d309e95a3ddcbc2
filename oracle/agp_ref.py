"""
oracle/agp_ref.py -- CPU restatement (NumPy/SciPy, fp64) of the SVGP + AnalyticVI/AnalyticSVI
hot path of AugmentedGaussianProcesses.jl v0.11.6.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke() and the
`cpu_baseline` leg of bench.py may import it -- as the checker (or as the timed CPU baseline),
never as the shipped compute path.  The product path (augmentedgaussianprocesses.jl_amd/) must
never import this module.

PARITY STATUS: "parity unpinned" against the literal reference.  The reference is pure Julia and
neither `julia` nor a Julia depot exists in the build container or on the GPU box, and the
reference's own tests hold no numeric golden values for this path.
What pins this restatement instead:
  * line-by-line citations below (file:line relative to /root/reference),
  * closed-form known-answer tests in tests/test_oracle_kat.py (Titsias optimum after one
    full-batch Gaussian step, exact-GP limit Z = X, utils identities of test/functions/utils.jl,
    one-hot answers of test/likelihood/multiclass.jl, mpmath tables, ELBO monotonicity,
    finite-difference check of the hyper-gradient),
  * the reference's behavioural thresholds (test/testingtools.jl:223-253) on its own toy set-ups,
  * an independent third-party implementation where one is installed (tests/test_oracle_third_party.py:
    kernel definitions against scikit-learn's RBF / Matern, the Gaussian path with Z = X against
    GaussianProcessRegressor -- predictions, proba_y, ELBO = exact log marginal likelihood).

Third-party arithmetic that is NOT under /root/reference and is restated from the published
definitions: KernelFunctions.jl (compat 0.8-0.10; SqExponential / Matern / ScaleTransform /
ARDTransform / ScaledKernel), LinearAlgebra (LAPACK potrf/trsm/potri via scipy),
Optimisers.jl Descent/ADAM, SpecialFunctions.digamma/loggamma (scipy.special),
FastGaussQuadrature.gausshermite(100) (numpy.polynomial.hermite.hermgauss).

All matrices are NumPy row-major arrays; X is (N, D) with one point per row (obsdim = 1,
`RowVecs`, src/data/datacontainer.jl:64-66).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import scipy.linalg as sla
from scipy.special import digamma, gammaln

LOG2 = math.log(2.0)
LOG2PI = math.log(2.0 * math.pi)


# --------------------------------------------------------------------------------------------
# src/functions/utils.jl
# --------------------------------------------------------------------------------------------
def jitt(dtype=np.float64) -> float:
    """src/functions/utils.jl:4-13 : 1e-4 (Float64), 1e-3 (Float32), 1e-2 (Float16)."""
    dt = np.dtype(dtype)
    if dt == np.float64:
        return 1e-4
    if dt == np.float32:
        return 1e-3
    if dt == np.float16:
        return 1e-2
    raise TypeError(dt)


def sqrt_expec_square(mu, s2, y=None):
    """src/functions/utils.jl:22-29."""
    if y is None:
        return np.sqrt(np.abs(mu) ** 2 + s2)
    return np.sqrt(np.abs(mu - y) ** 2 + s2)


def delta(i, j):
    """src/functions/utils.jl:32-35."""
    return 1.0 if i == j else 0.0


def hadamard(A, B):
    """src/functions/utils.jl:38-40."""
    return A * B


def add_transpose(A):
    """src/functions/utils.jl:43-45."""
    return A + A.T


def invquad(L, x):
    """src/functions/utils.jl:47 : sum(abs2, a.L \\ x) ; L = lower Cholesky factor."""
    return float(np.sum(sla.solve_triangular(L, x, lower=True) ** 2))


def trace_ABt(A, B):
    """src/functions/utils.jl:50-52."""
    return float(np.sum(A * B))


def diag_ABt(A, B):
    """src/functions/utils.jl:55-57 : vec(sum(A .* B; dims=2))."""
    return np.sum(A * B, axis=1)


def diagv_B(v, B):
    """src/functions/utils.jl:60-62."""
    return v[:, None] * B


def kappa_diag_theta_kappa(kappa, theta):
    """src/functions/utils.jl:65-67 : transpose(theta .* kappa) * kappa."""
    return (theta[:, None] * kappa).T @ kappa


def rho_kappa_diag_theta_kappa(rho, kappa, theta):
    """src/functions/utils.jl:70-72 : transpose((rho*theta) .* kappa) * kappa."""
    return ((rho * theta)[:, None] * kappa).T @ kappa


def opt_add_diag_mat(v, B):
    """src/functions/utils.jl:75-81."""
    A = B.copy()
    A[np.diag_indices_from(A)] += v
    return A


def logistic(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    pos = x >= 0
    out[pos] = 1.0 / (1.0 + np.exp(-x[pos]))
    e = np.exp(x[~pos])
    out[~pos] = e / (1.0 + e)
    return out


def safe_expcosh(mu, c):
    """src/functions/utils.jl:84-86 : exp(mu)/cosh(c), 2*logistic(2*max(mu,c)) if non-finite."""
    mu = np.asarray(mu, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = np.exp(mu) / np.cosh(c)
    bad = ~np.isfinite(r)
    if np.any(bad):
        r = np.where(bad, 2.0 * logistic(2.0 * np.maximum(mu, c)), r)
    return r


def logcosh(c):
    """src/functions/utils.jl:89-91 : log(exp(-2c)+1) + c - log 2."""
    c = np.asarray(c, dtype=np.float64)
    return np.log(np.exp(-2.0 * c) + 1.0) + c - LOG2


def theta_pg(c):
    """E[omega] of PG(1,c): tanh(c/2)/(2c) (src/likelihood/logistic.jl:47-49), limit 1/4 at c->0."""
    c = np.asarray(c, dtype=np.float64)
    small = np.abs(c) < 1e-6
    cs = np.where(small, 1.0, c)
    val = np.tanh(cs / 2.0) / (2.0 * cs)
    return np.where(small, 0.25 - c * c / 48.0, val)


# --------------------------------------------------------------------------------------------
# KernelFunctions.jl (third party, restated from its documented definitions; call sites
# src/gpblocks/latentgp.jl:202,206,210,212 ; src/training/predictions.jl:33,41,46)
# --------------------------------------------------------------------------------------------
@dataclass
class Kernel:
    """sigma2 * base( scale .* x , scale .* y ).

    kind: "sqexponential" exp(-d2/2)            (KernelFunctions SqExponentialKernel)
          "matern52"      (1+sqrt5 d+5d2/3)exp(-sqrt5 d)
          "matern32"      (1+sqrt3 d)exp(-sqrt3 d)
          "exponential"   exp(-d)
    scale: scalar (ScaleTransform(s)) or length-D vector (ARDTransform(v)).
    sigma2: ScaledKernel variance (`sigma2 * k`).
    """

    kind: str = "sqexponential"
    scale: object = 1.0
    sigma2: float = 1.0
    # structure of the Julia kernel object: `sigma2 * k` (ScaledKernel) / `k o ScaleTransform|ARDTransform`.  The reference's
    # hyper step is structural (Zygote NamedTuple over the object, autotuning.jl:99-118 -> update_kernel!,
    # autotuning_utils.jl:47-67): a parameter that is not part of the object is never stepped.
    has_variance: bool = True
    has_transform: bool = True

    def _scaled(self, X):
        return np.asarray(X, dtype=np.float64) * np.asarray(self.scale, dtype=np.float64)

    def base_from_d2(self, d2):
        d2 = np.maximum(d2, 0.0)
        if self.kind == "sqexponential":
            return np.exp(-0.5 * d2)
        d = np.sqrt(d2)
        if self.kind == "matern52":
            s5 = math.sqrt(5.0)
            return (1.0 + s5 * d + 5.0 * d2 / 3.0) * np.exp(-s5 * d)
        if self.kind == "matern32":
            s3 = math.sqrt(3.0)
            return (1.0 + s3 * d) * np.exp(-s3 * d)
        if self.kind == "exponential":
            return np.exp(-d)
        raise ValueError(self.kind)

    fast: bool = False  # CPU-baseline mode: GEMM form of the pairwise distances (what Distances.jl/BLAS does)

    def matrix(self, X, Y=None):
        """kernelmatrix(k, X[, Y]) with direct pairwise squared distances (no GEMM trick) unless self.fast."""
        Xs = self._scaled(X)
        Ys = Xs if Y is None else self._scaled(Y)
        if self.fast:
            d2 = (np.sum(Xs * Xs, axis=1)[:, None] + np.sum(Ys * Ys, axis=1)[None, :]) - 2.0 * (Xs @ Ys.T)
            return self.sigma2 * self.base_from_d2(d2)
        d2 = np.zeros((Xs.shape[0], Ys.shape[0]))
        for d in range(Xs.shape[1]):
            diff = Xs[:, d][:, None] - Ys[:, d][None, :]
            d2 += diff * diff
        return self.sigma2 * self.base_from_d2(d2)

    def diag(self, X):
        """kernelmatrix_diag: stationary kernels -> sigma2."""
        return np.full(np.asarray(X).shape[0], self.sigma2, dtype=np.float64)


# --------------------------------------------------------------------------------------------
# Likelihoods (src/likelihood/*.jl)
# --------------------------------------------------------------------------------------------
@dataclass
class GaussianLikelihood:
    """src/likelihood/gaussian.jl.  opt_noise: an Adam (defined below) or None -- gaussian.jl:18-23; the step itself is in
    local_updates (gaussian.jl:56-72; `Optimisers.apply!` there is the removed in-place form of the `apply` this port states)."""

    sigma2: float = 1e-3
    n_latent: int = 1
    name: str = "gaussian"
    opt_noise: object = None


@dataclass
class LogisticLikelihood:
    """src/likelihood/logistic.jl, classification.jl."""

    n_latent: int = 1
    name: str = "logistic"


@dataclass
class StudentTLikelihood:
    """src/likelihood/studentt.jl:23-31 ; alpha = (nu+1)/2."""

    nu: float = 3.0
    sigma: float = 1.0
    n_latent: int = 1
    name: str = "studentt"

    @property
    def alpha(self):
        return (self.nu + 1.0) / 2.0


@dataclass
class LogisticSoftMaxLikelihood:
    """src/likelihood/logisticsoftmax.jl + multiclass.jl ; n_latent = n_class."""

    n_class: int = 3
    class_mapping: Optional[list] = None
    name: str = "logisticsoftmax"

    @property
    def n_latent(self):
        return self.n_class


@dataclass
class LaplaceLikelihood:
    """src/likelihood/laplace.jl:17-25 ; a = beta^-2, p = 1/2 (GIG parameters of q(omega))."""

    beta: float = 1.0
    n_latent: int = 1
    name: str = "laplace"

    @property
    def a(self):
        return self.beta ** -2


@dataclass
class BayesianSVM:
    """src/likelihood/bayesiansvm.jl:19-23 : BernoulliLikelihood(SVMLink())."""

    n_latent: int = 1
    name: str = "bayesiansvm"


@dataclass
class PoissonLikelihood:
    """src/likelihood/poisson.jl:16-24 : PoissonLikelihood(ScaledLogistic([lambda])); lambda is STATE: it is re-estimated
    at the end of every local update (poisson.jl:78)."""

    lam: float = 1.0
    n_latent: int = 1
    name: str = "poisson"


@dataclass
class NegBinomialLikelihood:
    """src/likelihood/negativebinomial.jl:22-27 (LogisticLink, r failures)."""

    r: float = 10.0
    n_latent: int = 1
    name: str = "negbinomial"


@dataclass
class HeteroscedasticLikelihood:
    """src/likelihood/heteroscedastic.jl:17-27 : HeteroscedasticGaussianLikelihood(InvScaledLogistic([lambda])),
    two latents (f, g) ; lambda is STATE (heteroscedastic.jl:95)."""

    lam: float = 1.0
    n_latent: int = 2
    name: str = "heteroscedastic"


def treat_labels(y, lik):
    """treat_labels! : classification.jl:29-44, regression.jl:10-15, multiclass.jl:40-94, event.jl:7-13."""
    if lik.name in ("gaussian", "studentt", "laplace", "heteroscedastic"):
        return np.asarray(y, dtype=np.float64)
    if lik.name in ("poisson", "negbinomial"):
        ya = np.asarray(y)
        if not np.issubdtype(ya.dtype, np.integer):
            raise ValueError("For event count target(s) should be integers")
        return ya.astype(np.float64)
    if lik.name in ("logistic", "bayesiansvm"):
        y = np.asarray(y)
        labels = sorted(int(v) for v in np.unique(y))
        if labels == [0, 1]:
            return np.sign(y.astype(np.float64) - 0.5)
        if labels == [-1, 1]:
            return y.astype(np.float64)
        raise ValueError("Labels of y should be binary {-1,1} or {0,1}")
    if lik.name == "logisticsoftmax":
        y = list(np.asarray(y).tolist()) if not isinstance(y, list) else y
        create_mapping(lik, y)
        return create_one_hot(lik, y)
    raise ValueError(lik.name)


def create_mapping(lik: LogisticSoftMaxLikelihood, y):
    """src/likelihood/multiclass.jl:60-78 (first-occurrence order, collapse to 1:K if subset)."""
    K = lik.n_class
    if lik.class_mapping is None:
        seen = []
        for v in y:
            if v not in seen:
                seen.append(v)
        cm = seen
        if len(cm) <= K and all((isinstance(v, (int, np.integer)) and 1 <= v <= K) for v in cm):
            cm = list(range(1, K + 1))
        elif len(cm) > K:
            raise RuntimeError("The number of unique labels in the data is not of the same size "
                               "then the predefined class number")
        lik.class_mapping = cm
    lik.ind_mapping = {v: i + 1 for i, v in enumerate(lik.class_mapping)}
    return lik.ind_mapping


def create_one_hot(lik: LogisticSoftMaxLikelihood, y):
    """src/likelihood/multiclass.jl:81-94."""
    for v in y:
        if v not in lik.class_mapping:
            raise RuntimeError("Some labels of y are not part of the expect labels")
    Y = np.zeros((len(y), lik.n_class), dtype=bool)
    for i, v in enumerate(y):
        for j in range(lik.n_class):
            if v == lik.class_mapping[j]:
                Y[i, j] = True
                break
    return Y


def init_local_vars(lik, B, rng=None):
    """init_local_vars: gaussian.jl:47-54, classification.jl:10-12, studentt.jl:64-66,
    logisticsoftmax.jl:43-53.  The `rand` initial values are all overwritten by the first
    local update before being read, except the LogisticSoftMax alpha (= K) which is state."""
    rng = rng or np.random.default_rng(0)
    if lik.name == "gaussian":
        lv = {"theta": np.full(B, 1.0 / lik.sigma2)}
        if lik.opt_noise is not None:  # gaussian.jl:49-52
            lv["state_sigma2"] = lik.opt_noise.init(np.zeros(1))
        return lv
    if lik.name in ("logistic", "studentt", "bayesiansvm", "negbinomial"):
        return {"c": rng.random(B), "theta": np.zeros(B)}
    if lik.name == "laplace":  # laplace.jl:56-58
        return {"b": rng.random(B), "theta": np.zeros(B)}
    if lik.name == "poisson":  # poisson.jl:60-62
        return {"c": rng.random(B), "theta": np.zeros(B), "gamma": rng.random(B)}
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:49-61
        return {k: np.ones(B) for k in ("c", "phi", "gamma", "theta", "sigg")}
    if lik.name == "logisticsoftmax":
        K = lik.n_class
        return {
            "c": [np.ones(B) for _ in range(K)],
            "alpha": K * np.ones(B),
            "beta": K * np.ones(B),
            "theta": [rng.random(B) * 2 for _ in range(K)],
            "gamma": [rng.random(B) for _ in range(K)],
        }
    raise ValueError(lik.name)


def local_updates(lv, lik, y, mu_f, var_f):
    """local_updates! : gaussian.jl:56-72, logistic.jl:39-51, studentt.jl:68-82,
    logisticsoftmax.jl:55-79.  mu_f/var_f are tuples (one entry per latent)."""
    if lik.name == "gaussian":
        if lik.opt_noise is not None:  # gaussian.jl:63-69: one optimiser step on log sigma2, ascent
            grad = ((np.sum(np.abs(y - mu_f[0]) ** 2) + np.sum(var_f[0])) / lik.sigma2 - len(y)) / 2.0
            lv["state_sigma2"], gradlog = lik.opt_noise.apply(lv["state_sigma2"], np.array([grad]))
            lik.sigma2 = float(np.exp(np.log(lik.sigma2) + gradlog[0]))
        lv["theta"] = np.full(len(y), 1.0 / lik.sigma2)
        return lv
    if lik.name == "logistic":
        c = sqrt_expec_square(mu_f[0], var_f[0])
        lv["c"] = c
        lv["theta"] = theta_pg(c)
        return lv
    if lik.name == "studentt":
        c = (np.abs(mu_f[0] - y) ** 2 + var_f[0] + lik.sigma ** 2 * lik.nu) / 2.0
        lv["c"] = c
        lv["theta"] = lik.alpha / c
        return lv
    if lik.name == "laplace":  # laplace.jl:60-73
        b = sqrt_expec_square(mu_f[0], var_f[0], y)
        lv["b"] = b
        lv["theta"] = math.sqrt(lik.a) / b
        return lv
    if lik.name == "bayesiansvm":  # bayesiansvm.jl:43-55
        c = np.abs(1.0 - y * mu_f[0]) ** 2 + var_f[0]
        lv["c"] = c
        lv["theta"] = 1.0 / np.sqrt(c)
        return lv
    if lik.name == "poisson":  # poisson.jl:64-80 (theta has no 1/2: mirrored as written)
        lam = lik.lam
        c = sqrt_expec_square(mu_f[0], var_f[0])
        lv["c"] = c
        lv["gamma"] = lam * safe_expcosh(-mu_f[0] / 2.0, c / 2.0) / 2.0
        lv["theta"] = (y + lv["gamma"]) / c * np.tanh(c / 2.0)
        lik.lam = float(np.sum(y) / np.sum(expectation_logistic(mu_f[0], var_f[0])))
        return lv
    if lik.name == "negbinomial":  # negativebinomial.jl:69-81
        c = sqrt_expec_square(mu_f[0], var_f[0])
        lv["c"] = c
        lv["theta"] = (lik.r + y) * np.tanh(c / 2.0) / c
        return lv
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:71-97 ; latent 0 is f, latent 1 is g
        lam = lik.lam
        lv["phi"] = (np.abs(mu_f[0] - y) ** 2 + var_f[0]) / 2.0
        lv["c"] = sqrt_expec_square(mu_f[1], var_f[1])
        lv["sigg"] = safe_expcosh(-mu_f[1] / 2.0, lv["c"] / 2.0) / 2.0
        lv["gamma"] = lam * lv["phi"] * lv["sigg"]
        lv["theta"] = (0.5 + lv["gamma"]) * np.tanh(lv["c"] / 2.0) / (2.0 * lv["c"])
        lik.lam = float(max(len(y) / (2.0 * np.dot(lv["phi"], 1.0 - lv["sigg"])), lam))
        return lv
    if lik.name == "logisticsoftmax":
        K = lik.n_class
        lv["c"] = [sqrt_expec_square(mu_f[k], var_f[k]) for k in range(K)]
        for _ in range(2):  # logisticsoftmax.jl:65-72
            psi = digamma(lv["alpha"])
            lv["gamma"] = [
                np.exp(psi) * safe_expcosh(-mu_f[k] / 2.0, lv["c"][k] / 2.0) / (2.0 * lv["beta"])
                for k in range(K)
            ]
            lv["alpha"] = 1.0 + sum(lv["gamma"])
        lv["theta"] = [
            (y[:, k].astype(np.float64) + lv["gamma"][k]) * theta_pg(lv["c"][k]) for k in range(K)
        ]
        return lv
    raise ValueError(lik.name)


def grad_E_mu(lik, y, lv):
    """grad E_mu : gaussian.jl:74-76, logistic.jl:64-66, studentt.jl:96, logisticsoftmax.jl:98-100."""
    if lik.name == "gaussian":
        return (y / lik.sigma2,)
    if lik.name == "logistic":
        return (y / 2.0,)
    if lik.name == "studentt":
        return (lv["theta"] * y,)
    if lik.name == "logisticsoftmax":
        return tuple((y[:, k].astype(np.float64) - lv["gamma"][k]) / 2.0 for k in range(lik.n_class))
    if lik.name == "laplace":  # laplace.jl:85-87
        return (lv["theta"] * y,)
    if lik.name == "bayesiansvm":  # bayesiansvm.jl:57-61
        return (y * (lv["theta"] + 1.0),)
    if lik.name == "poisson":  # poisson.jl:94-98
        return ((y - lv["gamma"]) / 2.0,)
    if lik.name == "negbinomial":  # negativebinomial.jl:94-96
        return ((y - lik.r) / 2.0,)
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:113-120 (lambda already updated by local_updates!)
        return (y * lik.lam * lv["sigg"] / 2.0, (0.5 - lv["gamma"]) / 2.0)
    raise ValueError(lik.name)


def grad_E_Sigma(lik, y, lv):
    """grad E_Sigma = theta/2 for all four : gaussian.jl:78-80, logistic.jl:67-69,
    studentt.jl:97-99, logisticsoftmax.jl:101-103."""
    if lik.name == "logisticsoftmax":
        return tuple(lv["theta"][k] / 2.0 for k in range(lik.n_class))
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:122-129
        return (lik.lam * lv["sigg"] / 2.0, lv["theta"] / 2.0)
    return (lv["theta"] / 2.0,)  # also laplace.jl:88-90, bayesiansvm.jl:63-67, poisson.jl:99-103, negativebinomial.jl:97-99


def expec_loglikelihood(lik, y, mu_f, var_f, lv, elbo_mode="corrected"):
    """expec_loglikelihood : gaussian.jl:82-93, logistic.jl:73-84, studentt.jl:103-119,
    logisticsoftmax.jl:106-115.
    elbo_mode="reference" reproduces logistic.jl:82 literally (dot(theta, mu));
    "corrected" uses dot(theta, mu.^2) as the docstring logistic.jl:12-16 requires (Appendix A Q2).
    """
    if lik.name == "gaussian":
        n = len(y)
        return -(n * (LOG2PI + math.log(lik.sigma2))
                 + (np.sum((y - mu_f[0]) ** 2) + np.sum(var_f[0])) / lik.sigma2) / 2.0
    if lik.name == "logistic":
        th = lv["theta"]
        mu = mu_f[0]
        tot = -len(y) * LOG2 / 2.0
        quad = np.dot(th, mu) if elbo_mode == "reference" else np.dot(th, mu * mu)
        tot += (np.dot(mu, y) - np.dot(th, var_f[0]) - quad) / 2.0
        return tot
    if lik.name == "studentt":
        th, c, mu = lv["theta"], lv["c"], mu_f[0]
        tot = -len(y) * math.log(2.0 * math.pi * lik.sigma ** 2) / 2.0
        tot += -np.sum(np.log(c) - digamma(lik.alpha))
        tot += -(np.dot(th, var_f[0]) + np.dot(th, mu * mu) - 2.0 * np.dot(th, mu * y)
                 + np.dot(th, y * y)) / 2.0
        return tot
    if lik.name == "logisticsoftmax":
        K = lik.n_class
        Y = y.astype(np.float64)
        tot = -Y.size * LOG2  # length(y) of the B x K one-hot view (Q16)
        tot += -sum(np.sum(lv["gamma"][k] + Y[:, k]) for k in range(K)) * LOG2
        s = 0.0
        for k in range(K):
            s += (np.dot(mu_f[k], Y[:, k] - lv["gamma"][k]) - np.dot(lv["theta"][k], mu_f[k] ** 2)
                  - np.dot(lv["theta"][k], var_f[k]))
        tot += s / 2.0
        return tot
    if lik.name == "laplace":  # laplace.jl:93-110
        th, mu = lv["theta"], mu_f[0]
        tot = -len(y) * LOG2PI / 2.0 + np.sum(np.log(th)) / 2.0
        tot += -(np.dot(th, var_f[0]) + np.dot(th, mu * mu) - 2.0 * np.dot(th, mu * y) + np.dot(th, y * y)) / 2.0
        return tot
    if lik.name == "bayesiansvm":
        # bayesiansvm.jl:71-83 ; "reference": + dot(theta, (1 - y mu)^2) exactly as written (line 81);
        # "corrected": -1/2 dot(theta, (1 - y mu)^2), the expectation of -(1 + w - y f)^2 / (2 w) (docstring :14-16)
        th, mu = lv["theta"], mu_f[0]
        q = np.dot(th, (1.0 - y * mu) ** 2)
        tot = -len(y) * LOG2 / 2.0 + np.dot(mu, y) - np.dot(th, var_f[0]) / 2.0
        tot += q if elbo_mode == "reference" else -q / 2.0
        return tot
    if lik.name == "poisson":  # poisson.jl:106-120 (lambda = the value left by the last local update)
        th, mu, g = lv["theta"], mu_f[0], lv["gamma"]
        tot = (np.dot(mu, y - g) - np.dot(th, mu * mu) - np.dot(th, var_f[0])) / 2.0
        tot += np.sum(y * math.log(lik.lam)) - np.sum(gammaln(y + 1.0)) - LOG2 * np.sum(y + g)
        return tot
    if lik.name == "negbinomial":
        # negativebinomial.jl:116-127 ; "reference": dot(theta, mu)/2 as written (line 125); "corrected": dot(theta, mu^2)/2
        th, mu = lv["theta"], mu_f[0]
        logconst = gammaln(y + lik.r) - gammaln(y + 1.0) - gammaln(lik.r)  # negbin_logconst :105-113
        tot = np.sum(logconst) - LOG2 * np.sum(y + lik.r)
        quad = np.dot(th, mu) if elbo_mode == "reference" else np.dot(th, mu * mu)
        tot += np.dot(mu, y - lik.r) / 2.0 - quad / 2.0 - np.dot(th, var_f[0]) / 2.0
        return tot
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:142-158 + PoissonKL :166-175
        lam = lik.lam
        tot = len(y) * (math.log(lam) / 2.0 - math.log(2.0 * math.sqrt(2.0 * math.pi)))
        tot += (np.dot(mu_f[1], 0.5 - lv["gamma"]) - np.dot(mu_f[1] ** 2, lv["theta"])
                - np.dot(var_f[1], lv["theta"])) / 2.0
        lam0 = lam * ((y - mu_f[0]) ** 2 + var_f[0]) / 2.0
        tot -= poisson_kl(lv["gamma"], lam0, np.log(lam0))
        return tot
    raise ValueError(lik.name)


def expectation_logistic(mu, s2):
    """expectation(logistic, mu, sigma2) : src/functions/utils.jl:16-19 (Gauss-Hermite 100, predictions.jl:4)."""
    nodes, weights = gauss_hermite_100()
    x = nodes[None, :] * np.sqrt(np.maximum(s2, 0.0))[:, None] + np.asarray(mu)[:, None]
    return logistic(x) @ weights


def log2besselk_half(s):
    """log(2 K_{1/2}(s)) with K_{1/2}(s) = sqrt(pi / (2 s)) exp(-s) (closed form of besselk(0.5, s))."""
    return LOG2 + 0.5 * (np.log(np.pi) - LOG2 - np.log(s)) - s


# src/functions/KLdivergences.jl ------------------------------------------------------------
def gaussian_kl(mu, mu0, Sigma, L):
    """KLdivergences.jl:11-18 ; L = lower Cholesky factor of K."""
    m = len(mu)
    logdetK = 2.0 * np.sum(np.log(np.diag(L)))
    sign, logdetS = np.linalg.slogdet(Sigma)
    KinvS = sla.cho_solve((L, True), Sigma)
    return (logdetK - logdetS + np.trace(KinvS) + invquad(L, mu - mu0) - m) / 2.0


def polya_gamma_kl(b, c, theta):
    """KLdivergences.jl:96-98."""
    return float(np.dot(b, logcosh(c / 2.0)) - np.dot(c * c, theta) / 2.0)


def gamma_kl(alpha, beta, alpha_p, beta_p):
    """KLdivergences.jl:62-67 (broadcast sum; alpha scalar, beta vector in the StudentT use)."""
    beta = np.asarray(beta, dtype=np.float64)
    return float(np.sum((alpha - alpha_p) * digamma(alpha) - gammaln(alpha) + gammaln(alpha_p)
                        + alpha_p * (np.log(beta) - np.log(beta_p)) + alpha * (beta_p - beta) / beta))


def xlogx(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0)), 0.0)


def poisson_kl(lam, lam0, psi):
    """KLdivergences.jl:83-89."""
    return float(np.sum(lam0) - np.sum(lam) + np.sum(xlogx(lam)) - np.dot(lam, psi))


def augmented_kl(lik, lv, y, mode="corrected"):
    """AugmentedKL : gaussian.jl:95 (0), logistic.jl:86-92, studentt.jl:121-127,
    logisticsoftmax.jl:117-140."""
    if lik.name == "gaussian":
        return 0.0
    if lik.name == "logistic":
        c = lv["c"]
        return polya_gamma_kl(np.ones_like(c), c, lv["theta"])
    if lik.name == "studentt":
        alpha_p = lik.nu / 2.0
        beta_p = alpha_p * lik.sigma ** 2
        return gamma_kl(lik.alpha, lv["c"], alpha_p, beta_p)
    if lik.name == "logisticsoftmax":
        K = lik.n_class
        Y = y.astype(np.float64)
        pg = sum(polya_gamma_kl(Y[:, k] + lv["gamma"][k], lv["c"][k], lv["theta"][k]) for k in range(K))
        lam0 = lv["alpha"] / lv["beta"]
        psi = digamma(lv["alpha"]) - np.log(lv["beta"])
        po = sum(poisson_kl(lv["gamma"][k], lam0, psi) for k in range(K))
        a = lv["alpha"]
        # GammaEntropy logisticsoftmax.jl:136-140 : sum(log, first(beta)) == log(beta[1]) (Q16)
        ge = (-np.sum(a) + math.log(lv["beta"][0]) - np.sum(gammaln(a)) - np.dot(1.0 - a, digamma(a)))
        return float(pg + po + ge)
    if lik.name == "laplace":
        # laplace.jl:112-123 + GIGEntropy KLdivergences.jl:105-113 with (a, b, p) = (beta^-2, b.^2, 1/2).  For p = 1/2:
        # K_{3/2}(s) = K_{1/2}(s)(1 + 1/s), K_{-1/2} = K_{1/2}  =>  s/K_p (K_{p+1} + K_{p-1}) / 2 = s + 1/2.
        # "reference" keeps two Julia iteration quirks of GIGEntropy with a scalar a and p: sum(log, a) = log(a) ONCE and
        # mapreduce(f, +, p, sqrt_ab) zips the scalar p with the vector => only the FIRST point's log(2 K_p) enters.
        a, b = lik.a, lv["b"]
        sab = np.sqrt(a * b * b)
        n = len(b)
        if mode == "reference":
            ent = (math.log(a) - np.sum(np.log(b * b))) / 2.0 + float(log2besselk_half(sab[:1])[0]) + np.sum(sab + 0.5)
        else:
            ent = (n * math.log(a) - np.sum(np.log(b * b))) / 2.0 + np.sum(log2besselk_half(sab)) + np.sum(sab + 0.5)
        expo = np.sum(-math.log(2.0 * lik.beta ** 2) - (a * b + b * b * math.sqrt(a)) / (a * b * b * lik.beta ** 2) / 2.0)
        return float(ent - expo)
    if lik.name == "bayesiansvm":  # bayesiansvm.jl:85-92
        c = lv["c"]
        return float(np.sum(np.log(c)) / 2.0 + np.sum(log2besselk_half(np.sqrt(c))) - np.sum(np.sqrt(c)) / 2.0)
    if lik.name == "poisson":  # poisson.jl:122-132 ; PoissonKL(lambda vec, lambda0 scalar) KLdivergences.jl:74-76
        g, lam0 = lv["gamma"], lik.lam
        pk = lam0 * len(g) - (1.0 + math.log(lam0)) * np.sum(g) + np.sum(xlogx(g))
        return float(pk + polya_gamma_kl(y + g, lv["c"], lv["theta"]))
    if lik.name == "negbinomial":  # negativebinomial.jl:103,129-131
        return polya_gamma_kl(y + lik.r, lv["c"], lv["theta"])
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:160-164,177-179
        return polya_gamma_kl(0.5 + lv["gamma"], lv["c"], lv["theta"])
    raise ValueError(lik.name)


# --------------------------------------------------------------------------------------------
# GP blocks (src/gpblocks/latentgp.jl, posterior.jl) and inference (src/inference/*.jl)
# --------------------------------------------------------------------------------------------
class NotPosDef(Exception):
    """Julia PosDefException from cholesky (latentgp.jl:206)."""


class NegativeKtilde(Exception):
    """error("K~ has negative values") latentgp.jl:213."""


def compute_K(kernel: Kernel, Z, jitter):
    """compute_K latentgp.jl:205-207 : cholesky(kernelmatrix(k, Z) + jitt*I) -> (K, L lower)."""
    K = kernel.matrix(Z) + jitter * np.eye(len(Z))
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError as e:  # pragma: no cover
        raise NotPosDef(str(e))
    return K, L


def compute_kappa(kernel: Kernel, X, Z, L, jitter):
    """compute_kappa latentgp.jl:209-215."""
    Knm = kernel.matrix(X, Z)
    kappa = sla.cho_solve((L, True), Knm.T).T  # Knm / K
    Kt = kernel.diag(X) + jitter - diag_ABt(kappa, Knm)
    if not np.all(Kt > 0):
        raise NegativeKtilde("K~ has negative values")
    return Knm, kappa, Kt


def mean_f(mu, kappa):
    """latentgp.jl:179."""
    return kappa @ mu


def var_f(Sigma, kappa, Kt):
    """latentgp.jl:189 : diag_ABt(kappa*Sigma, kappa) + K~."""
    return diag_ABt(kappa @ Sigma, kappa) + Kt


def grad_eta1(gmu, rho, kappa, L, mu0, eta1):
    """analyticVI.jl:160-169."""
    return kappa.T @ (rho * gmu) + sla.cho_solve((L, True), mu0) - eta1


def grad_eta2(gS, rho, kappa, Kinv, eta2):
    """analyticVI.jl:172-180 ; inv(K) passed in (the reference recomputes it every call)."""
    return -(rho_kappa_diag_theta_kappa(rho, kappa, gS) + Kinv / 2.0) - eta2


def robbins_monro_lr(n, kappa_rm=0.51, tau=1.0):
    """optimisers.jl:14-19 with state n (init 1, optimisers.jl:12): Delta/(tau+n)^kappa."""
    return 1.0 / (tau + n) ** kappa_rm


def natural_to_standard(eta1, eta2):
    """inference.jl:25-28 : Sigma = -inv(eta2)/2 ; mu = Sigma*eta1."""
    Sigma = -np.linalg.inv(eta2) / 2.0
    Sigma = (Sigma + Sigma.T) / 2.0  # Symmetric wrapper
    return Sigma @ eta1, Sigma


@dataclass
class Latent:
    """SparseVarLatent (latentgp.jl:44-70) + VarPosterior init (posterior.jl:29-37)."""

    kernel: Kernel
    Z: np.ndarray
    mu0: Optional[np.ndarray] = None  # ZeroMean -> zeros
    mu: np.ndarray = None
    Sigma: np.ndarray = None
    eta1: np.ndarray = None
    eta2: np.ndarray = None
    # kernel matrices ("state.kernel_matrices")
    K: np.ndarray = None
    L: np.ndarray = None
    Kinv: np.ndarray = None
    Knm: np.ndarray = None
    kappa: np.ndarray = None
    Kt: np.ndarray = None
    # opt state
    n_eta1: int = 1
    n_eta2: int = 1

    def __post_init__(self):
        m = len(self.Z)
        self.Z = np.array(self.Z, dtype=np.float64)
        if self.mu0 is None:
            self.mu0 = np.zeros(m)
        self.mu = np.zeros(m)
        self.Sigma = np.eye(m)
        self.eta1 = np.zeros(m)
        self.eta2 = -0.5 * np.eye(m)


@dataclass
class SVGP:
    """src/models/SVGP.jl:22-80 + AnalyticVI state (analyticVI.jl:1-52).

    stochastic=False -> AnalyticVI() (Descent(1.0) step, rho = 1)
    stochastic=True  -> AnalyticSVI(batchsize) with RobbinsMonro(kappa_rm, tau).
    Each latent owns a deep copy of kernel and Z (latentgp.jl:63-68).
    """

    kernel: Kernel
    likelihood: object
    Z: np.ndarray
    stochastic: bool = False
    batchsize: int = 0
    kappa_rm: float = 0.51
    tau_rm: float = 1.0
    jitter: float = 1e-4
    elbo_mode: str = "corrected"
    latents: list = field(default_factory=list)
    local_vars: dict = None
    rho: float = 1.0
    n_iter: int = 0
    hp_updated: bool = True
    # hyper-parameter optimisation (SVGP(...; optimiser, Zoptimiser, atfrequency) SVGP.jl:39-42): Adam objects or None
    k_opt: object = None
    z_opt: object = None
    ard: bool = False          # True: the scale is an ARDTransform vector (one parameter per dim), else ScaleTransform
    atfrequency: int = 1
    hyper_state: list = None
    reference_compat_stale_K: bool = False

    def __post_init__(self):
        import copy
        kernels = self.kernel if isinstance(self.kernel, (list, tuple)) else None
        self.latents = [
            Latent(copy.deepcopy(kernels[k] if kernels else self.kernel), np.array(self.Z, dtype=np.float64))
            for k in range(self.likelihood.n_latent)
        ]

    # -- training.jl:187-208 ---------------------------------------------------------------
    def compute_kernel_matrices(self, X, update=False):
        for gp in self.latents:
            if self.hp_updated or update:
                gp.K, gp.L = compute_K(gp.kernel, gp.Z, self.jitter)
                gp.Kinv = sla.cho_solve((gp.L, True), np.eye(len(gp.Z)))
                gp.Kinv = (gp.Kinv + gp.Kinv.T) / 2.0
            if self.hp_updated or self.stochastic or update:
                gp.Knm, gp.kappa, gp.Kt = compute_kappa(gp.kernel, X, gp.Z, gp.L, self.jitter)
        self.hp_updated = False

    def mean_f(self):
        return tuple(mean_f(gp.mu, gp.kappa) for gp in self.latents)

    def var_f(self):
        return tuple(var_f(gp.Sigma, gp.kappa, gp.Kt) for gp in self.latents)

    # -- analyticVI.jl:62-85 -------------------------------------------------------------
    def variational_updates(self, y):
        if self.local_vars is None:
            self.local_vars = init_local_vars(self.likelihood, len(y))
        lv = local_updates(self.local_vars, self.likelihood, y, self.mean_f(), self.var_f())
        self.local_vars = lv
        g1 = grad_E_mu(self.likelihood, y, lv)
        g2 = grad_E_Sigma(self.likelihood, y, lv)
        for k, gp in enumerate(self.latents):
            d1 = grad_eta1(g1[k], self.rho, gp.kappa, gp.L, gp.mu0, gp.eta1)
            d2 = grad_eta2(g2[k], self.rho, gp.kappa, gp.Kinv, gp.eta2)
            # global_update! analyticVI.jl:229-246
            if self.stochastic:
                lr1 = robbins_monro_lr(gp.n_eta1, self.kappa_rm, self.tau_rm)
                lr2 = robbins_monro_lr(gp.n_eta2, self.kappa_rm, self.tau_rm)
                gp.n_eta1 += 1
                gp.n_eta2 += 1
                gp.eta1 = gp.eta1 + lr1 * d1
                gp.eta2 = lr2 * d2 + gp.eta2
            else:
                gp.eta1 = gp.eta1 + d1
                gp.eta2 = d2 + gp.eta2
            gp.eta2 = (gp.eta2 + gp.eta2.T) / 2.0
            gp.mu, gp.Sigma = natural_to_standard(gp.eta1, gp.eta2)

    # -- training.jl:140-144 ------------------------------------------------------------
    def update_parameters(self, X, y):
        self.compute_kernel_matrices(X)
        self.variational_updates(y)

    # -- training.jl:13-111 (fixed iteration count, indices supplied by the caller) ------------
    def train(self, X, y, iterations, idx_stream: Optional[Sequence[np.ndarray]] = None, callback=None,
              labels_treated=False, fresh_state=True):
        X = np.asarray(X, dtype=np.float64)
        y = y if labels_treated else treat_labels(y, self.likelihood)
        N = len(X)
        if self.stochastic:
            if not (0 < self.batchsize <= N):
                raise ValueError("The size of mini-batch is incorrect")
            self.rho = N / self.batchsize
        else:
            self.batchsize = N
            self.rho = 1.0
        if fresh_state:
            self.hp_updated = True  # training.jl:41-43 (state === nothing)
        for it in range(iterations):
            if self.stochastic:
                idx = np.asarray(idx_stream[it])
                xb, yb = X[idx], y[idx]
            else:
                xb, yb = X, y
            self.update_parameters(xb, yb)
            if callback is not None:
                callback(self, it, xb, yb)
            # training.jl:65-69 : n_iter is the counter BEFORE this iteration's increment
            if (self.k_opt or self.z_opt) and self.n_iter % self.atfrequency == 0 and self.n_iter >= 3 \
                    and (it + 1) != iterations:
                self.update_hyperparameters(xb, yb)
            self.n_iter += 1
        # compute_Ks training.jl:107,210-215
        for gp in self.latents:
            gp.K, gp.L = compute_K(gp.kernel, gp.Z, self.jitter)
        return self

    # -- autotuning.jl:86-140 + autotuning_utils.jl:47-82 (ADAM ascent; positive parameters stepped in log space) ----
    def update_hyperparameters(self, xb, yb):
        if self.hyper_state is None:
            self.hyper_state = [None] * len(self.latents)
        for k, gp in enumerate(self.latents):
            g = hyper_gradient(self, xb, yb, k, self.rho)
            D = gp.Z.shape[1]
            sc = np.broadcast_to(np.asarray(gp.kernel.scale, dtype=np.float64), (D,)).copy()
            if self.hyper_state[k] is None:
                self.hyper_state[k] = {
                    "var": self.k_opt.init(np.zeros(1)) if self.k_opt else None,
                    "scale": self.k_opt.init(np.zeros(D if self.ard else 1)) if self.k_opt else None,
                    "Z": self.z_opt.init(np.zeros_like(gp.Z)) if self.z_opt else None,
                }
            st = self.hyper_state[k]
            if self.k_opt:
                if getattr(gp.kernel, "has_variance", True):
                    v = np.array([gp.kernel.sigma2])
                    st["var"], dv = self.k_opt.apply(st["var"], v * np.array([g["dvariance"]]))
                    gp.kernel.sigma2 = float(np.exp(np.log(v) + dv)[0])
                if not getattr(gp.kernel, "has_transform", True):
                    pass  # a bare kernel: no scale parameter exists
                elif self.ard:
                    st["scale"], ds = self.k_opt.apply(st["scale"], sc * g["dscale"])
                    gp.kernel.scale = np.exp(np.log(sc) + ds)
                else:
                    s0 = np.array([sc[0]])
                    st["scale"], ds = self.k_opt.apply(st["scale"], s0 * np.array([np.sum(g["dscale"])]))
                    gp.kernel.scale = float(np.exp(np.log(s0) + ds)[0])
            if self.z_opt:
                st["Z"], dz = self.z_opt.apply(st["Z"], g["dZ"])
                gp.Z = gp.Z + dz
        # the reference never sets HyperParametersUpdated again inside train! (the call is commented out, autotuning.jl:41-46),
        # so K = chol(K_ZZ) stays the one of the first iteration until train! ends (Appendix A Q1).  Corrected by default.
        if not self.reference_compat_stale_K:
            self.hp_updated = True

    # -- analyticVI.jl:255-274 ----------------------------------------------------------
    def elbo(self, y, rho=None):
        """ELBO(model, state, y) on the kernel matrices / local vars currently in the state."""
        rho = self.rho if rho is None else rho
        tot = rho * expec_loglikelihood(self.likelihood, y, self.mean_f(), self.var_f(),
                                        self.local_vars, self.elbo_mode)
        tot -= sum(gaussian_kl(gp.mu, gp.mu0, gp.Sigma, gp.L) for gp in self.latents)
        tot -= rho * augmented_kl(self.likelihood, self.local_vars, y, self.elbo_mode)
        return float(tot)

    def elbo_fresh(self, X, y, rho):
        """External ELBO(model, X, y) (src/functions/ELBO.jl:32-47): recompute kernel matrices on
        (X, y), re-init local vars at that size, ONE local update, then ELBO; rho explicit (Q13)."""
        save = (self.local_vars, [(gp.Knm, gp.kappa, gp.Kt) for gp in self.latents], self.hp_updated)
        self.compute_kernel_matrices(np.asarray(X, dtype=np.float64), update=True)
        self.local_vars = init_local_vars(self.likelihood, len(y))
        self.local_vars = local_updates(self.local_vars, self.likelihood, y, self.mean_f(), self.var_f())
        val = self.elbo(y, rho)
        self.local_vars = save[0]
        for gp, (a, b, c) in zip(self.latents, save[1]):
            gp.Knm, gp.kappa, gp.Kt = a, b, c
        self.hp_updated = save[2]
        return val

    # -- predictions.jl:25-50 -----------------------------------------------------------
    def predict_f(self, Xt, cov=False, diag=True):
        """_predict_f (sparse) predictions.jl:25-50.  diag=False: full covariance k** + jitt I - k* A k*' (lines 45-49)."""
        Xt = np.asarray(Xt, dtype=np.float64)
        mus, vars_ = [], []
        for gp in self.latents:
            K, L = compute_K(gp.kernel, gp.Z, self.jitter) if gp.L is None else (gp.K, gp.L)
            ks = gp.kernel.matrix(Xt, gp.Z)
            mus.append(ks @ sla.cho_solve((L, True), gp.mu))
            if cov:
                m = len(gp.Z)
                SK = sla.cho_solve((L, True), gp.Sigma.T).T  # Sigma / K
                A = sla.cho_solve((L, True), np.eye(m) - SK)  # K \ (I - Sigma/K)
                if not diag:
                    kss_full = gp.kernel.matrix(Xt) + self.jitter * np.eye(len(Xt))
                    vars_.append(kss_full - ks @ A @ ks.T)
                    continue
                kss = gp.kernel.diag(Xt) + self.jitter
                vars_.append(kss - diag_ABt(ks @ A, ks))
        if cov:
            return tuple(mus), tuple(vars_)
        return tuple(mus)

    def predict_y(self, Xt):
        """predictions.jl:178-198 + regression.jl:17-18, classification.jl:47-48."""
        mu = self.predict_f(Xt, cov=False)
        lik = self.likelihood
        if lik.name in ("gaussian", "studentt", "laplace", "heteroscedastic"):
            return mu[0]  # regression.jl:17-18 ; heteroscedastic.jl:137-141 (first latent)
        if lik.name in ("logistic", "bayesiansvm"):
            return mu[0] > 0
        if lik.name == "poisson":  # predictions.jl:211 : mean(Poisson(lambda logistic(mu)))
            return lik.lam * logistic(mu[0])
        if lik.name == "negbinomial":  # mean(NegativeBinomial(r, logistic(-mu))) = r (1 - p)/p = r exp(mu)
            p = logistic(-mu[0])
            return lik.r * (1.0 - p) / p
        if lik.name == "logisticsoftmax":
            am = np.argmax(np.stack(mu, axis=1), axis=1)
            cm = lik.class_mapping or list(range(1, lik.n_class + 1))
            return np.array([cm[i] for i in am], dtype=object if not isinstance(cm[0], (int, np.integer)) else np.int64)
        raise ValueError(lik.name)

    def proba_y(self, Xt):
        """predictions.jl:225-247 + compute_proba per likelihood."""
        mu, var = self.predict_f(Xt, cov=True)
        return compute_proba(self.likelihood, mu, var)


_GH = None


def gauss_hermite_100():
    """predictions.jl:4 : (x*sqrt2, w/sqrt(pi)) from gausshermite(100)."""
    global _GH
    if _GH is None:
        x, w = np.polynomial.hermite.hermgauss(100)
        _GH = (x * math.sqrt(2.0), w / math.sqrt(math.pi))
    return _GH


def compute_proba(lik, mu, var):
    """gaussian.jl:41-45 ; studentt.jl:57-61 ; classification.jl:14-26 ; multiclass.jl:96-117 +
    logisticsoftmax.jl:29-31."""
    if lik.name == "gaussian":
        return mu[0], var[0] + lik.sigma2
    if lik.name == "studentt":
        return mu[0], np.maximum(var[0], 0.0) + lik.nu * lik.sigma ** 2 / (2.0 * (lik.nu / 2.0 - 1.0))
    if lik.name == "logistic":
        nodes, weights = gauss_hermite_100()
        x = nodes[None, :] * np.sqrt(np.maximum(var[0], 0.0))[:, None] + mu[0][:, None]
        s = logistic(x)
        pred = s @ weights
        v = np.maximum((s * s) @ weights - pred ** 2, 0.0)
        return pred, v
    if lik.name == "logisticsoftmax":
        s = logistic(np.stack(mu, axis=1))
        return s / np.sum(np.abs(s), axis=1, keepdims=True)
    if lik.name == "laplace":  # laplace.jl:48-52
        return mu[0], np.maximum(var[0], 0.0) + 2.0 * lik.beta ** 2
    if lik.name == "heteroscedastic":  # heteroscedastic.jl:63-69
        return mu[0], var[0] + 1.0 / (lik.lam * logistic(mu[1]))
    if lik.name in ("bayesiansvm", "poisson", "negbinomial"):
        nodes, weights = gauss_hermite_100()
        x = nodes[None, :] * np.sqrt(np.maximum(var[0], 0.0))[:, None] + mu[0][:, None]
        if lik.name == "bayesiansvm":  # classification.jl:14-26 with SVMLink (bayesiansvm.jl:27-40)
            pos = np.exp(-2.0 * np.maximum(1.0 - x, 0.0))
            neg = np.exp(-2.0 * np.maximum(1.0 + x, 0.0))
            s = pos / (pos + neg)
            pred = s @ weights
            return pred, np.maximum((s * s) @ weights - pred ** 2, 0.0)
        if lik.name == "poisson":  # poisson.jl:46-57
            s = lik.lam * logistic(x)
        else:  # negativebinomial.jl:46-62
            p = logistic(x)
            s = p * lik.r / (1.0 - p)
        pred = s @ weights
        return pred, (s * s) @ weights - pred ** 2
    raise ValueError(lik.name)


# --------------------------------------------------------------------------------------------
# Hyper-parameter gradient (src/hyperparameter/autotuning.jl:86-140 differentiates
# ELBO(model, x, y, mu0, ks, Zs, state) of src/functions/ELBO.jl:15-21 with (mu, Sigma, local
# vars) held fixed and AugmentedKL ignored (analyticVI.jl:269-271)).  The oracle evaluates that
# objective as a plain function of (log-scale, log-variance, Z); tests differentiate it by central
# finite differences to pin the hand-written HIP backward.
# --------------------------------------------------------------------------------------------
def hyper_objective(model: SVGP, X, y, latent_k, scale, sigma2, Z, rho):
    import copy
    gp = model.latents[latent_k]
    ker = copy.deepcopy(gp.kernel)
    ker.scale, ker.sigma2 = scale, sigma2
    K, L = compute_K(ker, Z, model.jitter)
    Knm, kappa, Kt = compute_kappa(ker, X, Z, L, model.jitter)
    mus, vs = [], []
    for k, g in enumerate(model.latents):
        if k == latent_k:
            mus.append(mean_f(g.mu, kappa))
            vs.append(var_f(g.Sigma, kappa, Kt))
        else:
            mus.append(mean_f(g.mu, g.kappa))
            vs.append(var_f(g.Sigma, g.kappa, g.Kt))
    tot = rho * expec_loglikelihood(model.likelihood, y, tuple(mus), tuple(vs), model.local_vars,
                                    model.elbo_mode)
    for k, g in enumerate(model.latents):
        Lk = L if k == latent_k else g.L
        tot -= gaussian_kl(g.mu, g.mu0, g.Sigma, Lk)
    return float(tot)


# --------------------------------------------------------------------------------------------
# Multi-output sparse model (src/models/MOSVGP.jl, src/models/single_and_multi_output_utils.jl:24-118,
# src/inference/analyticVI.jl:87-111,277-297, src/training/training.jl:153-158, predictions.jl:52-92).
# Q latent GPs are mixed into n_task outputs f_t = sum_q A[t][q] f_q (nf_per_task = 1 for the likelihoods on this
# path).  The reference confuses n_output (= Q) with the number of tasks (MOSVGP.jl:126, Appendix A Q7) and is only
# self-consistent for Q == n_task; the loops below run over TASKS, the documented intent (docs/src/userguide.md:44).
# --------------------------------------------------------------------------------------------
@dataclass
class Adam:
    """Optimisers.jl ADAM(eta, (0.9, 0.999)) with bias correction, eps = 1e-8 [unvendored; stated, SURVEY 3.5]."""
    eta: float = 0.01
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8

    def init(self, x):
        return {"m": np.zeros_like(x), "v": np.zeros_like(x), "t": 0}

    def apply(self, st, g):
        st["t"] += 1
        st["m"] = self.b1 * st["m"] + (1 - self.b1) * g
        st["v"] = self.b2 * st["v"] + (1 - self.b2) * g * g
        mh = st["m"] / (1 - self.b1 ** st["t"])
        vh = st["v"] / (1 - self.b2 ** st["t"])
        return st, self.eta * mh / (np.sqrt(vh) + self.eps)


@dataclass
class Descent:
    """Optimisers.jl Descent(eta): dx' = eta dx [unvendored; the package's documented rule].  The reference hands whatever rule
    it is given to Optimisers.apply and ADDS dx' (src/hyperparameter/autotuning_utils.jl:63-76)."""
    eta: float = 0.1

    def init(self, x):
        return {}

    def apply(self, st, g):
        return st, self.eta * g


@dataclass
class Momentum:
    """Optimisers.jl Momentum(eta, rho): vel = rho vel + eta dx ; dx' = vel [unvendored; the package's documented rule]."""
    eta: float = 0.01
    rho: float = 0.9

    def init(self, x):
        return {"vel": np.zeros_like(x)}

    def apply(self, st, g):
        st["vel"] = self.rho * st["vel"] + self.eta * g
        return st, st["vel"].copy()


def init_local_vars_single(lik, B):
    """theta / c as the positional buffers of init_local_vars (classification.jl:10-12 etc.), with the `rand` entries that
    are always overwritten before use set to zero."""
    if lik.name == "gaussian":
        return {"theta": np.full(B, 1.0 / lik.sigma2), "c": np.zeros(B)}
    return {"theta": np.zeros(B), "c": np.zeros(B)}


@dataclass
class MOSVGP:
    kernel: object
    likelihoods: list
    Zs: list                      # one (m, D) array per latent
    A: np.ndarray                 # (n_task, Q) mixing weights (rows normalised, MOSVGP.jl:101-104)
    stochastic: bool = False
    batchsize: int = 0
    A_opt: Optional[Adam] = None  # Aoptimiser (None == false)
    kappa_rm: float = 0.51
    tau_rm: float = 1.0
    jitter: float = 1e-4
    elbo_mode: str = "corrected"
    k_opt: object = None          # optimiser / Zoptimiser of MOSVGP(...) (MOSVGP.jl:39-42): Adam objects or None
    z_opt: object = None
    ard: bool = False
    atfrequency: int = 1

    def __post_init__(self):
        import copy
        kernels = self.kernel if isinstance(self.kernel, (list, tuple)) else [self.kernel]
        self.latents = [Latent(copy.deepcopy(kernels[i % len(kernels)]), np.array(Z, dtype=np.float64))
                        for i, Z in enumerate(self.Zs)]  # kernel[mod1(i, n_kernel)] MOSVGP.jl:96-98
        self.A = np.array(self.A, dtype=np.float64)
        self.n_task, self.Q = self.A.shape
        assert len(self.likelihoods) == self.n_task and len(self.latents) == self.Q
        for l in self.likelihoods:
            assert l.name in ("gaussian", "logistic", "studentt", "laplace", "bayesiansvm", "negbinomial")
        self.local_vars = None
        self.A_state = [self.A_opt.init(self.A[t]) for t in range(self.n_task)] if self.A_opt else None
        self.rho = 1.0
        self.hp_updated = True
        self.n_iter = 0

    compute_kernel_matrices = SVGP.compute_kernel_matrices

    def lat_mean_var(self):
        return ([mean_f(g.mu, g.kappa) for g in self.latents],
                [var_f(g.Sigma, g.kappa, g.Kt) for g in self.latents])

    def mixed(self):
        mu_q, var_q = self.lat_mean_var()
        mu_t = [sum(self.A[t, q] * mu_q[q] for q in range(self.Q)) for t in range(self.n_task)]
        var_t = [sum(self.A[t, q] ** 2 * var_q[q] for q in range(self.Q)) for t in range(self.n_task)]
        return mu_t, var_t

    def update_A(self, ys):
        """update_A! single_and_multi_output_utils.jl:87-118 (uses the local variables of the PREVIOUS step)."""
        if self.A_opt is None:
            return
        mu_q, var_q = self.lat_mean_var()
        for t, lik in enumerate(self.likelihoods):
            gmu = grad_E_mu(lik, ys[t], self.local_vars[t])[0]
            gS = grad_E_Sigma(lik, ys[t], self.local_vars[t])[0]
            dA = np.zeros(self.Q)
            for q in range(self.Q):
                others = sum(self.A[t, qq] * mu_q[qq] for qq in range(self.Q) if qq != q)
                x1 = np.dot(gmu, mu_q[q]) - 2.0 * np.dot(gS, mu_q[q] * others)
                x2 = np.dot(gS, mu_q[q] ** 2 + var_q[q])
                dA[q] = x1 - 2.0 * self.A[t, q] * x2
            self.A_state[t], delta = self.A_opt.apply(self.A_state[t], dA)
            self.A[t] = self.A[t] + delta
            self.A[t] = self.A[t] / math.sqrt(np.sum(self.A[t] ** 2))

    def variational_updates(self, ys):
        """analyticVI.jl:87-111 with the mixed gradients of single_and_multi_output_utils.jl:48-84."""
        mu_q, var_q = self.lat_mean_var()
        mu_t, var_t = self.mixed()
        for t, lik in enumerate(self.likelihoods):
            self.local_vars[t] = local_updates(self.local_vars[t], lik, ys[t], (mu_t[t],), (var_t[t],))
        gmu = [grad_E_mu(l, ys[t], self.local_vars[t])[0] for t, l in enumerate(self.likelihoods)]
        gS = [grad_E_Sigma(l, ys[t], self.local_vars[t])[0] for t, l in enumerate(self.likelihoods)]
        for q, gp in enumerate(self.latents):
            g1 = sum(self.A[t, q] * (gmu[t] - 2.0 * gS[t] * (mu_t[t] - self.A[t, q] * mu_q[q]))
                     for t in range(self.n_task))
            g2 = sum(self.A[t, q] ** 2 * gS[t] for t in range(self.n_task))
            d1 = grad_eta1(g1, self.rho, gp.kappa, gp.L, gp.mu0, gp.eta1)
            d2 = grad_eta2(g2, self.rho, gp.kappa, gp.Kinv, gp.eta2)
            lr = robbins_monro_lr(gp.n_eta1, self.kappa_rm, self.tau_rm) if self.stochastic else 1.0
            gp.n_eta1 += 1
            gp.n_eta2 += 1
            gp.eta1 = gp.eta1 + lr * d1
            gp.eta2 = gp.eta2 + lr * d2
            gp.eta2 = (gp.eta2 + gp.eta2.T) / 2.0
            gp.mu, gp.Sigma = natural_to_standard(gp.eta1, gp.eta2)

    def train(self, X, ys, iterations, idx_stream=None, callback=None):
        """train! + update_parameters!(::MOSVGP) training.jl:153-158.  ys: list of treated target vectors (one per task)."""
        X = np.asarray(X, dtype=np.float64)
        N = len(X)
        if self.stochastic:
            self.rho = N / self.batchsize
        else:
            self.batchsize = N
            self.rho = 1.0
        B = self.batchsize
        if self.local_vars is None:
            self.local_vars = [init_local_vars_single(l, B) for l in self.likelihoods]
        for it in range(iterations):
            idx = np.asarray(idx_stream[it]) if self.stochastic else np.arange(N)
            xb, yb = X[idx], [y[idx] for y in ys]
            self.compute_kernel_matrices(xb)
            self.update_A(yb)
            self.variational_updates(yb)
            if callback is not None:
                callback(self, it, xb, yb)
            if (self.k_opt or self.z_opt) and self.n_iter % self.atfrequency == 0 and self.n_iter >= 3 \
                    and (it + 1) != iterations:  # training.jl:65-69
                self.update_hyperparameters(xb, yb)
            self.n_iter += 1
        for gp in self.latents:
            gp.K, gp.L = compute_K(gp.kernel, gp.Z, self.jitter)
        return self

    # -- update_hyperparameters! (sparse, autotuning.jl:86-140) for the multi-output model: the data term sees latent q through
    #    the mixed means / variances, so dE/dmu_q = sum_t A_tq dE_t/dmu_t and dE/dsigma2_q = sum_t A_tq^2 dE_t/dsigma2_t
    def hyper_gradient(self, xb, ys, q):
        self.hp_updated = True
        self.compute_kernel_matrices(xb)
        mu_t, _ = self.mixed()
        gmu, gsig = np.zeros(len(xb)), np.zeros(len(xb))
        for t, lik in enumerate(self.likelihoods):
            gm, gs = expec_grads(lik, ys[t], mu_t[t], self.local_vars[t], 0, self.elbo_mode)
            gmu += self.A[t, q] * gm
            gsig += self.A[t, q] ** 2 * gs
        return hyper_gradient_core(self.latents[q], xb, gmu, gsig, self.rho, self.jitter)

    def hyper_objective(self, xb, ys, q, scale, sigma2, Z):
        """ELBO.jl:15-21 as a function of latent q's kernel parameters and inducing points ((mu, Sigma, local variables, A)
        fixed, AugmentedKL ignored): what autotuning.jl:96-98 hands to Zygote; finite differences of it pin hyper_gradient."""
        import copy
        mus, vs = [], []
        kl = 0.0
        for k, g in enumerate(self.latents):
            ker, Zk = g.kernel, g.Z
            if k == q:
                ker = copy.deepcopy(ker)
                ker.scale, ker.sigma2 = scale, sigma2
                Zk = Z
            K, L = compute_K(ker, Zk, self.jitter)
            Knm, kappa, Kt = compute_kappa(ker, xb, Zk, L, self.jitter)
            mus.append(mean_f(g.mu, kappa))
            vs.append(var_f(g.Sigma, kappa, Kt))
            kl += gaussian_kl(g.mu, g.mu0, g.Sigma, L)
        tot = 0.0
        for t, lik in enumerate(self.likelihoods):
            mt = sum(self.A[t, k] * mus[k] for k in range(self.Q))
            vt = sum(self.A[t, k] ** 2 * vs[k] for k in range(self.Q))
            tot += expec_loglikelihood(lik, ys[t], (mt,), (vt,), self.local_vars[t], self.elbo_mode)
        return float(self.rho * tot - kl)

    def update_hyperparameters(self, xb, ys):
        if getattr(self, "hyper_state", None) is None:
            self.hyper_state = [None] * self.Q
        grads = [self.hyper_gradient(xb, ys, q) for q in range(self.Q)]  # all gradients at the same state
        for q, gp in enumerate(self.latents):
            g = grads[q]
            D = gp.Z.shape[1]
            sc = np.broadcast_to(np.asarray(gp.kernel.scale, dtype=np.float64), (D,)).copy()
            if self.hyper_state[q] is None:
                self.hyper_state[q] = {"var": self.k_opt.init(np.zeros(1)) if self.k_opt else None,
                                       "scale": self.k_opt.init(np.zeros(D if self.ard else 1)) if self.k_opt else None,
                                       "Z": self.z_opt.init(np.zeros_like(gp.Z)) if self.z_opt else None}
            st = self.hyper_state[q]
            if self.k_opt:
                if getattr(gp.kernel, "has_variance", True):
                    v = np.array([gp.kernel.sigma2])
                    st["var"], dv = self.k_opt.apply(st["var"], v * np.array([g["dvariance"]]))
                    gp.kernel.sigma2 = float(np.exp(np.log(v) + dv)[0])
                if not getattr(gp.kernel, "has_transform", True):
                    pass  # a bare kernel: no scale parameter exists
                elif self.ard:
                    st["scale"], ds = self.k_opt.apply(st["scale"], sc * g["dscale"])
                    gp.kernel.scale = np.exp(np.log(sc) + ds)
                else:
                    s0 = np.array([sc[0]])
                    st["scale"], ds = self.k_opt.apply(st["scale"], s0 * np.array([np.sum(g["dscale"])]))
                    gp.kernel.scale = float(np.exp(np.log(s0) + ds)[0])
            if self.z_opt:
                st["Z"], dz = self.z_opt.apply(st["Z"], g["dZ"])
                gp.Z = gp.Z + dz
        self.hp_updated = True

    def elbo(self, ys, rho=None):
        """analyticVI.jl:277-297."""
        rho = self.rho if rho is None else rho
        mu_t, var_t = self.mixed()
        tot = rho * sum(expec_loglikelihood(l, ys[t], (mu_t[t],), (var_t[t],), self.local_vars[t], self.elbo_mode)
                        for t, l in enumerate(self.likelihoods))
        tot -= sum(gaussian_kl(gp.mu, gp.mu0, gp.Sigma, gp.L) for gp in self.latents)
        tot -= rho * sum(augmented_kl(l, self.local_vars[t], ys[t], self.elbo_mode)
                         for t, l in enumerate(self.likelihoods))
        return float(tot)

    def predict_f(self, Xt, cov=False, diag=True):
        """predictions.jl:52-92: latent predictions mixed by A (means by A, variances / full covariances (diag=False, :82-90) by
        A^2)."""
        helper = SVGP.__new__(SVGP)
        helper.latents, helper.jitter = self.latents, self.jitter
        if cov:
            mq, vq = SVGP.predict_f(helper, Xt, cov=True, diag=diag)
        else:
            mq, vq = SVGP.predict_f(helper, Xt, cov=False), None
        mu_t = [sum(self.A[t, q] * mq[q] for q in range(self.Q)) for t in range(self.n_task)]
        if not cov:
            return tuple(mu_t)
        var_t = [sum(self.A[t, q] ** 2 * vq[q] for q in range(self.Q)) for t in range(self.n_task)]
        return tuple(mu_t), tuple(var_t)

    def predict_y(self, Xt):
        mu = self.predict_f(Xt)
        out = []
        for m, l in zip(mu, self.likelihoods):  # predict_y.(likelihood(model), ...) predictions.jl:196
            if l.name in ("logistic", "bayesiansvm"):
                out.append(m > 0)
            elif l.name == "negbinomial":
                p = logistic(-m)
                out.append(l.r * (1.0 - p) / p)
            else:
                out.append(m)
        return out

    def proba_y(self, Xt):
        mu, var = self.predict_f(Xt, cov=True)
        return [compute_proba(l, (mu[t],), (var[t],)) for t, l in enumerate(self.likelihoods)]


# --------------------------------------------------------------------------------------------
# Analytic hyper-gradient of the objective the reference differentiates with Zygote
# (src/hyperparameter/autotuning.jl:86-140 over src/functions/ELBO.jl:15-21): ELBO as a function of the kernel parameters
# and Z of ONE latent with (mu, Sigma, local variables) fixed and AugmentedKL ignored.  Formula sheet: SURVEY.md 8(a15),
# re-derived here; pinned against central finite differences of hyper_objective in tests/test_oracle_kat.py.
# --------------------------------------------------------------------------------------------
def dphi_dd2(kind, d2):
    """d base(d2) / d d2 for the stationary base kernels (finite at d2 = 0 for SE / Matern)."""
    d2 = np.maximum(d2, 0.0)
    if kind == "sqexponential":
        return -0.5 * np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if kind == "matern52":
        s5 = math.sqrt(5.0)
        return -(5.0 / 6.0) * (1.0 + s5 * r) * np.exp(-s5 * r)
    if kind == "matern32":
        s3 = math.sqrt(3.0)
        return -1.5 * np.exp(-s3 * r)
    raise ValueError("hyper-gradients are defined for SqExponential / Matern32 / Matern52 here")


def expec_grads(lik, y, mu_f, lv, latent_k=0, elbo_mode="corrected", var_f=None):
    """(dE/dmu_f, dE/dsigma2_f) of expec_loglikelihood for one latent: g_mu = grad_E_mu - theta*mu_f, g_sigma = -theta/2
    (all four augmented likelihoods; the reference-bug logistic variant has g_mu = y/2 - theta/2)."""
    if lik.name == "heteroscedastic" and latent_k == 0:
        # d/d(mu_1, sigma2_1) of -PoissonKL(gamma, lambda0, log lambda0), lambda0 = lam ((y-mu_1)^2 + sigma2_1)/2 evaluated
        # at the CURRENT (mu_1, sigma2_1) with gamma fixed: t = lam - gamma / phi_now ; (-t (mu_1 - y), -t/2)
        t1 = lik.lam - lv["gamma"] / (((mu_f - y) ** 2 + var_f) / 2.0)
        return -t1 * (mu_f - y), -t1 / 2.0
    g1 = grad_E_mu(lik, y, lv)[latent_k]
    th = lv["theta"][latent_k] if lik.name == "logisticsoftmax" else lv["theta"]
    if lik.name in ("logistic", "negbinomial") and elbo_mode == "reference":
        return g1 - th / 2.0, -th / 2.0
    if lik.name == "bayesiansvm" and elbo_mode == "reference":
        return y - 2.0 * th * (1.0 - y * mu_f) * y, -th / 2.0
    return g1 - th * mu_f, -th / 2.0


def hyper_gradient(model, X, y, latent_k, rho):
    """Returns dict(dvariance, dscale (array, one per dim: sum it for a ScaleTransform), dZ) at the current state."""
    gp = model.latents[latent_k]
    ker, Z = gp.kernel, gp.Z
    K, L = compute_K(ker, Z, model.jitter)
    Knm, kappa, Kt = compute_kappa(ker, X, Z, L, model.jitter)
    mu_f = mean_f(gp.mu, kappa)
    gmu, gsig = expec_grads(model.likelihood, y, mu_f, model.local_vars, latent_k, model.elbo_mode,
                            var_f(gp.Sigma, kappa, Kt))
    return hyper_gradient_core(gp, X, gmu, gsig, rho, model.jitter)


def hyper_gradient_core(gp, X, gmu, gsig, rho, jitter, online=None):
    """the backward pass given (dE/dmu_f, dE/dsigma2_f) of the data term for this latent.
    online = dict(Za, invDa, prev_eta1): adds the gradient of -extraKL (KLdivergences.jl:30-54), which the reference's
    ELBO closure recomputes with the candidate kernel / Z through compute_kappa(::OnlineVarLatent) (latentgp.jl:217-237):
      E_x = 1/2 tr(D K~_a) + 1/2 tr(D kappa_a Sigma kappa_a') - eta_a' kappa_a mu + 1/2 mu' kappa_a' D kappa_a mu
      G_kappa_a = D kappa_a (Sigma + mu mu') - eta_a mu' - D K_ab / 2 ;  G_Kab = G_kappa_a K^-1 - D kappa_a / 2 ;
      G_K += -sym(kappa_a' G_kappa_a K^-1) ;  G_Ka = D / 2"""
    ker, Z = gp.kernel, gp.Z
    m = len(Z)
    K, L = compute_K(ker, Z, jitter)
    Kinv = sla.cho_solve((L, True), np.eye(m))
    Knm, kappa, Kt = compute_kappa(ker, X, Z, L, jitter)
    G_kappa = rho * (np.outer(gmu, gp.mu) + 2.0 * gsig[:, None] * (kappa @ gp.Sigma) - gsig[:, None] * Knm)
    H = G_kappa @ Kinv
    G_Knm = H - rho * gsig[:, None] * kappa
    G_kdiag = rho * gsig
    d = gp.mu - gp.mu0
    a = Kinv @ d
    M1 = kappa.T @ H
    G_K = -0.5 * (M1 + M1.T) - 0.5 * (Kinv - Kinv @ gp.Sigma @ Kinv) + 0.5 * np.outer(a, a)
    s = np.broadcast_to(np.asarray(ker.scale, dtype=np.float64), (X.shape[1],)).copy()

    def back(Gm, Xa, Zb):
        Xs, Zs_ = Xa * s, Zb * s
        diff = Xs[:, None, :] - Zs_[None, :, :]          # s_d (x_d - z_d)
        d2 = np.sum(diff * diff, axis=2)
        phi = ker.base_from_d2(d2)
        GK = Gm * ker.sigma2 * dphi_dd2(ker.kind, d2)     # dL/dd2
        dvar = np.sum(Gm * phi)
        dscale = 2.0 * np.einsum("ij,ijd->d", GK, diff * (Xa[:, None, :] - Zb[None, :, :]))
        dZcol = -2.0 * np.einsum("ij,ijd->jd", GK, diff) * s[None, :]
        return dvar, dscale, dZcol

    extra_v, extra_s, extra_z = 0.0, 0.0, 0.0
    if online is not None and online.get("Za") is not None:
        Za, Dm, ea = online["Za"], online["invDa"], online["prev_eta1"]
        Kab = ker.matrix(Za, Z)
        ka = Kab @ Kinv
        G_ka = Dm @ ka @ (gp.Sigma + np.outer(gp.mu, gp.mu)) - np.outer(ea, gp.mu) - 0.5 * Dm @ Kab
        HK = G_ka @ Kinv
        G_Kab = HK - 0.5 * Dm @ ka
        M2 = ka.T @ HK
        G_K = G_K - 0.5 * (M2 + M2.T)
        va, sa, za = back(G_Kab, Za, Z)
        vb, sb, _ = back(0.5 * Dm, Za, Za)
        extra_v, extra_s, extra_z = va + vb, sa + sb, za
    v1, s1, z1 = back(G_Knm, X, Z)
    v2, s2, z2 = back(G_K, Z, Z)
    return {"dvariance": v1 + v2 + np.sum(G_kdiag) + extra_v, "dscale": s1 + s2 + extra_s, "dZ": z1 + 2.0 * z2 + extra_z}


# --------------------------------------------------------------------------------------------
# Inducing-point selection: inducingpoints(KmeansAlg(m), X)  (call sites test/testingtools.jl:66,
# test/models/MOSVGP.jl:14, docs/examples/gpclassification.jl:47, docs/src/userguide.md:140-143).
# The algorithm is THIRD PARTY and unvendored: InducingPoints.jl (re-exported, src/AugmentedGaussianProcesses.jl:33; no
# pinned version) `kmeans_ip` = `kmeans_seeding` (the AFK-MC2 seeding of Bachem et al., "Fast and Provably Good Seedings for
# k-Means", NeurIPS 2016, with chain length nMarkov = 10) followed by Clustering.jl `kmeans!(X, C; tol = 1e-3)` (Lloyd).
# Restated from the published algorithms; parity unpinned (no reference test pins centres: they are random).
# --------------------------------------------------------------------------------------------
def nearest_center(X, C):
    """argmin_j ||x_i - c_j||^2 (ties -> smaller j) and the squared distance, from direct differences sum_d (x_id - c_jd)^2 in
    float64, accumulated one coordinate at a time."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    d = np.zeros((len(X), len(C)))
    Xt, Ct = np.ascontiguousarray(X.T), np.ascontiguousarray(C.T)
    for k in range(X.shape[1]):
        df = Xt[k][:, None] - Ct[k][None, :]
        df *= df
        d += df
    lab = np.argmin(d, axis=1)
    return lab.astype(np.int32), d[np.arange(len(X)), lab]


def kmeans_seeding(X, nC, n_markov, rng):
    """AFK-MC2 seeding as InducingPoints.jl's kmeans_seeding runs it: proposal q(x) = d(x, c1)^2 / (2 sum d^2) + 1/(2N);
    every further centre is the end of a length-n_markov Metropolis chain that accepts y over x when
    d(y, C)^2 / d(x, C)^2 > u.  Draw order (shared with the host mirror so that both see the same randomness):
    first index, then all proposal indices, then all uniforms."""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    first = int(rng.integers(N))
    q = np.sum((X - X[first]) ** 2, axis=1)
    q = q / np.sum(q) / 2.0 + 1.0 / (2.0 * N)
    q = q / np.sum(q)
    prop = rng.choice(N, size=(max(nC - 1, 0), n_markov), p=q)
    u = rng.random((max(nC - 1, 0), max(n_markov - 1, 0)))
    return seeding_chains(X[first], X[prop.ravel()].reshape(prop.shape + (X.shape[1],)), u)


def seeding_chains(x_first, cand, u):
    """the sequential part of kmeans_seeding on pre-drawn candidates cand[i, j] (point j of chain i) and uniforms u[i, j-1]"""
    C = [np.asarray(x_first, dtype=np.float64)]
    for i in range(cand.shape[0]):
        Cm = np.stack(C)
        x = cand[i, 0]
        mind = np.min(np.sum((Cm - x) ** 2, axis=1))
        for j in range(1, cand.shape[1]):
            y = cand[i, j]
            dist = np.min(np.sum((Cm - y) ** 2, axis=1))
            if dist > u[i, j - 1] * mind:  # dist / mindist > rand(), written without the division (mindist may be 0)
                x, mind = y, dist
        C.append(np.asarray(x, dtype=np.float64))
    return np.stack(C)


def kmeans_lloyd(X, C0, tol=1e-3, maxiter=100):
    """Clustering.kmeans! control flow: assign ; repeat { centres <- cluster means ; assign ; stop when the cost changed by
    less than tol (absolute) }.  A cluster that lost all its points keeps its centre (Clustering.jl re-seeds it at random;
    not reproduced).  Returns (centres, labels, iterations, cost, converged)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    lab, mind = nearest_center(X, C)
    obj = float(np.sum(mind))
    it, conv = 0, False
    while it < maxiter and not conv:
        it += 1
        for j in range(len(C)):
            msk = lab == j
            if np.any(msk):
                C[j] = X[msk].mean(axis=0)
        lab, mind = nearest_center(X, C)
        prev, obj = obj, float(np.sum(mind))
        conv = len(C) == 1 or abs(obj - prev) < tol
    return C, lab, it, obj, conv


def kmeans_inducingpoints(X, m, rng, n_markov=10, tol=1e-3):
    """inducingpoints(KmeansAlg(m; nMarkov = 10, tol = 1e-3), X)"""
    return kmeans_lloyd(X, kmeans_seeding(X, m, n_markov, rng), tol)[0]


# --------------------------------------------------------------------------------------------
# OnlineSVGP (src/models/OnlineSVGP.jl, src/training/onlinetraining.jl, latentgp.jl:90-131,217-237,
# analyticVI.jl:183-203, KLdivergences.jl:30-54, states.jl:85-97, posterior.jl:39-55): streaming sparse GP of
# Bui et al. 2017 with closed-form augmented updates.  Inducing points come from the third-party, unvendored
# InducingPoints.jl OIPS (Galy-Fajou & Opper 2021): restated below from the published algorithm (parity unpinned).
# --------------------------------------------------------------------------------------------
@dataclass
class OIPS:
    """Online Inducing Point Selection: a point joins Z when its largest kernel value with the current Z is below
    rho_accept; optional pruning (`remove_point`) drops one of the points whose kernel value with another inducing point
    exceeds rho_remove, drawn with weights = number of such neighbours (needs the caller's RNG; rho_remove >= 1 disables it)."""

    rho_accept: float = 0.8
    rho_remove: float = 1.0
    kmin: int = 10

    def init(self, X, kernel):
        """inducingpoints(alg, X; kernel): start from the first point, then add_point over the rest."""
        return self.update(np.asarray(X[:1], dtype=np.float64).copy(), X[1:], kernel)

    def update(self, Z, X, kernel):
        """updateZ(Z, alg, X; kernel): sequential scan, every accepted point is visible to the later ones."""
        Z = [z for z in np.asarray(Z, dtype=np.float64)]
        for x in np.asarray(X, dtype=np.float64):
            kx = kernel.matrix(x[None, :], np.stack(Z))[0]
            if np.max(kx) < self.rho_accept:
                Z.append(x.copy())
        return np.stack(Z)

    def remove_point(self, rng, Z, Kmat):
        if self.rho_remove >= 1.0:
            return Z
        overlap = np.sum(Kmat > self.rho_remove, axis=1) - 1
        removable = np.flatnonzero(overlap > 0)
        if len(removable) > 1 and len(Z) > self.kmin:
            w = overlap[removable].astype(np.float64)
            gone = removable[rng.choice(len(removable), p=w / w.sum())]
            return np.delete(Z, gone, axis=0)
        return Z


class OnlineSVGP:
    """OnlineSVGP(kernel, likelihood, AnalyticVI(), Zalg; optimiser=false): one `train` call per arriving batch."""

    def __init__(self, kernel, likelihood, Zalg=None, jitter=1e-4, elbo_mode="corrected", rng=None, k_opt=None, z_opt=None,
                 atfrequency=1):
        self.k_opt, self.z_opt, self.atfrequency = k_opt, z_opt, atfrequency
        self._hp_dirty = False
        self.kernel, self.likelihood, self.Zalg = kernel, likelihood, Zalg or OIPS(0.9)
        self.jitter, self.elbo_mode = jitter, elbo_mode
        self.rng = rng or np.random.default_rng(0)
        self.latents = None  # list of dicts, one per latent
        self.local_vars = None
        self.n_iter = 0
        self.rho = 1.0

    # -- init_online_gp! onlinetraining.jl:188-197 + OnlineVarPosterior posterior.jl:47-55 + init_opt_state states.jl:85-97
    def _init(self, X):
        import copy
        self.latents = []
        for _ in range(self.likelihood.n_latent):
            ker = copy.deepcopy(self.kernel)
            Z = self.Zalg.init(X, ker)
            k = len(Z)
            self.latents.append(dict(kernel=ker, Z=Z, Za=None, mu=np.zeros(k), Sigma=np.eye(k), eta1=np.zeros(k),
                                     eta2=-0.5 * np.eye(k), mu0=np.zeros(k), prevLa=0.0, invDa=np.eye(k), prev_eta1=np.zeros(k)))

    # -- save_old_gp! onlinetraining.jl:170-180 and updateZs! :153-160
    def _roll(self, X):
        for g in self.latents:
            g["Za"] = g["Z"].copy()
            g["Z"] = self.Zalg.remove_point(self.rng, g["Z"], g["K"])
            g["invDa"] = -2.0 * g["eta2"] - g["Kinv"]
            g["invDa"] = (g["invDa"] + g["invDa"].T) / 2.0
            g["prev_eta1"] = g["eta1"].copy()
            g["prevLa"] = float((-np.linalg.slogdet(g["Sigma"])[1] + 2.0 * np.sum(np.log(np.diag(g["L"])))
                                 - np.dot(g["mu"], g["eta1"])) / 2.0)
            g["Z"] = self.Zalg.update(g["Z"], X, g["kernel"])
            g["mu0"] = np.zeros(len(g["Z"]))
        for st in (getattr(self, "hyper_state", None) or []):
            if st is not None:
                st["Zshape"] = None  # the Z optimiser restarts with every arriving batch (its parameter array is a new one)

    # -- compute_old_matrices onlinetraining.jl:210-217 : matrices of the new batch w.r.t. the OLD inducing points
    def _old_matrices(self, X):
        out = []
        for g in self.latents:
            K, L = compute_K(g["kernel"], g["Za"], self.jitter)
            out.append(compute_kappa(g["kernel"], X, g["Za"], L, self.jitter))
        return out

    # -- compute_K + compute_kappa(::OnlineVarLatent) latentgp.jl:217-237
    def _matrices(self, X):
        for g in self.latents:
            ker, Z = g["kernel"], g["Z"]
            g["K"], g["L"] = compute_K(ker, Z, self.jitter)
            g["Kinv"] = sla.cho_solve((g["L"], True), np.eye(len(Z)))
            g["Kinv"] = (g["Kinv"] + g["Kinv"].T) / 2.0
            k = len(Z)
            if g["Za"] is None:
                g["Kab"], g["kappa_a"], g["Kt_a"] = np.zeros((k, k)), np.eye(k), np.zeros((k, k))
            else:
                g["Kab"] = ker.matrix(g["Za"], Z)
                g["kappa_a"] = sla.cho_solve((g["L"], True), g["Kab"].T).T
                Ka = ker.matrix(g["Za"]) + self.jitter * np.eye(len(g["Za"]))
                g["Kt_a"] = Ka - g["kappa_a"] @ g["Kab"].T
            g["Knm"], g["kappa"], g["Kt"] = compute_kappa(ker, X, Z, g["L"], self.jitter)

    # -- natural_gradient!(::OnlineVarLatent) analyticVI.jl:183-203 + global_update! :221-224
    def _natural(self, g1, g2):
        for k, g in enumerate(self.latents):
            ka = g["kappa_a"]
            g["eta1"] = sla.cho_solve((g["L"], True), g["mu0"]) + g["kappa"].T @ g1[k] + ka.T @ g["prev_eta1"]
            e2 = -(rho_kappa_diag_theta_kappa(1.0, g["kappa"], g2[k]) + ka.T @ g["invDa"] @ ka / 2.0 + g["Kinv"] / 2.0)
            g["eta2"] = (e2 + e2.T) / 2.0
            g["mu"], g["Sigma"] = natural_to_standard(g["eta1"], g["eta2"])

    def mean_var(self):
        return (tuple(mean_f(g["mu"], g["kappa"]) for g in self.latents),
                tuple(var_f(g["Sigma"], g["kappa"], g["Kt"]) for g in self.latents))

    # -- train!(::OnlineSVGP, X, y, state; iterations) onlinetraining.jl:36-135
    def train(self, X, y, iterations=5, callback=None):
        X = np.asarray(X, dtype=np.float64)
        lik = self.likelihood
        y = treat_labels(y, lik)
        B = len(X)
        first = self.n_iter == 0
        if first:
            self._init(X)
        else:
            self._roll(X)
        if self.local_vars is None or len(np.atleast_1d(_first_array(self.local_vars))) != B:
            self.local_vars = init_local_vars(lik, B)
        for it in range(iterations):
            if it == 0:
                if first:
                    self._matrices(X)
                    mf, vf = self.mean_var()
                else:
                    old = self._old_matrices(X)
                    mf = tuple(mean_f(g["mu"], o[1]) for g, o in zip(self.latents, old))
                    vf = tuple(var_f(g["Sigma"], o[1], o[2]) for g, o in zip(self.latents, old))
                self.local_vars = local_updates(self.local_vars, lik, y, mf, vf)
                g1, g2 = grad_E_mu(lik, y, self.local_vars), grad_E_Sigma(lik, y, self.local_vars)
                self._matrices(X)
            else:
                if self._hp_dirty:  # update_parameters! -> compute_kernel_matrices recomputes after a hyper step
                    self._matrices(X)
                    self._hp_dirty = False
                mf, vf = self.mean_var()
                self.local_vars = local_updates(self.local_vars, lik, y, mf, vf)
                g1, g2 = grad_E_mu(lik, y, self.local_vars), grad_E_Sigma(lik, y, self.local_vars)
            self._natural(g1, g2)
            if callback is not None:
                callback(self, it, X, y)
            # onlinetraining.jl:112-114 (n_iter is the counter before this iteration's increment)
            if (self.k_opt or self.z_opt) and self.n_iter % self.atfrequency == 0 and self.n_iter >= 3:
                self.update_hyperparameters(X, y)
            self.n_iter += 1
        if self._hp_dirty:  # final compute_kernel_matrices(m, state, X, true) onlinetraining.jl:133
            self._matrices(X)
            self._hp_dirty = False
        return self

    # -- update_hyperparameters! (sparse, autotuning.jl:86-140) on the online model: the differentiated ELBO includes extraKL
    def _latent_view(self, g):
        lt = Latent(g["kernel"], g["Z"])
        lt.mu, lt.Sigma, lt.mu0 = g["mu"], g["Sigma"], g["mu0"]
        return lt

    def hyper_gradient(self, X, y, l):
        g = self.latents[l]
        K, L = compute_K(g["kernel"], g["Z"], self.jitter)
        Knm, kappa, Kt = compute_kappa(g["kernel"], X, g["Z"], L, self.jitter)
        gmu, gsig = expec_grads(self.likelihood, y, mean_f(g["mu"], kappa), self.local_vars, l, self.elbo_mode,
                                var_f(g["Sigma"], kappa, Kt))
        return hyper_gradient_core(self._latent_view(g), X, gmu, gsig, 1.0, self.jitter,
                                   online=dict(Za=g["Za"], invDa=g["invDa"], prev_eta1=g["prev_eta1"]))

    def hyper_objective(self, X, y, l, scale, sigma2, Z):
        """ELBO.jl:15-21 for the online model as a function of latent l's kernel parameters and inducing points"""
        import copy
        keep = {k: self.latents[l][k] for k in ("kernel", "Z", "K", "L", "Kinv", "Kab", "kappa_a", "Kt_a", "Knm", "kappa", "Kt")}
        ker = copy.deepcopy(self.latents[l]["kernel"])
        ker.scale, ker.sigma2 = scale, sigma2
        self.latents[l]["kernel"], self.latents[l]["Z"] = ker, Z
        self._matrices(X)
        mf, vf = self.mean_var()
        val = expec_loglikelihood(self.likelihood, y, mf, vf, self.local_vars, self.elbo_mode)
        val -= sum(gaussian_kl(g["mu"], g["mu0"], g["Sigma"], g["L"]) for g in self.latents)
        val -= self.extra_kl()
        self.latents[l].update(keep)
        return float(val)

    def update_hyperparameters(self, X, y):
        grads = [self.hyper_gradient(X, y, l) for l in range(len(self.latents))]
        if getattr(self, "hyper_state", None) is None:
            self.hyper_state = [None] * len(self.latents)
        for l, g in enumerate(self.latents):
            gr = grads[l]
            D = g["Z"].shape[1]
            ker = g["kernel"]
            sc = np.broadcast_to(np.asarray(ker.scale, dtype=np.float64), (D,)).copy()
            ard = np.ndim(ker.scale) > 0
            st = self.hyper_state[l]
            if st is None or (self.z_opt and st["Z"] is not None and st["Zshape"] != g["Z"].shape):
                old = st
                st = {"var": old["var"] if old else (self.k_opt.init(np.zeros(1)) if self.k_opt else None),
                      "scale": old["scale"] if old else (self.k_opt.init(np.zeros(D if ard else 1)) if self.k_opt else None),
                      "Z": self.z_opt.init(np.zeros_like(g["Z"])) if self.z_opt else None, "Zshape": g["Z"].shape}
                self.hyper_state[l] = st
            if self.k_opt:
                v = np.array([ker.sigma2])
                st["var"], dv = self.k_opt.apply(st["var"], v * np.array([gr["dvariance"]]))
                ker.sigma2 = float(np.exp(np.log(v) + dv)[0])
                if ard:
                    st["scale"], ds = self.k_opt.apply(st["scale"], sc * gr["dscale"])
                    ker.scale = np.exp(np.log(sc) + ds)
                else:
                    s0 = np.array([sc[0]])
                    st["scale"], ds = self.k_opt.apply(st["scale"], s0 * np.array([np.sum(gr["dscale"])]))
                    ker.scale = float(np.exp(np.log(s0) + ds)[0])
            if self.z_opt:
                st["Z"], dz = self.z_opt.apply(st["Z"], gr["dZ"])
                g["Z"] = g["Z"] + dz
        self._hp_dirty = True

    # -- ELBO analyticVI.jl:255-274 with extraKL KLdivergences.jl:30-54
    def extra_kl(self):
        tot = 0.0
        for g in self.latents:
            ka, iD = g["kappa_a"], g["invDa"]
            kam = ka @ g["mu"]
            kl = g["prevLa"]
            kl += -(trace_ABt(iD, g["Kt_a"]) + trace_ABt(iD, ka @ g["Sigma"] @ ka.T)) / 2.0
            kl += np.dot(g["prev_eta1"], kam) - np.dot(kam, iD @ kam) / 2.0
            tot += kl
        return float(tot)

    def elbo(self, y):
        mf, vf = self.mean_var()
        tot = self.rho * expec_loglikelihood(self.likelihood, y, mf, vf, self.local_vars, self.elbo_mode)
        tot -= sum(gaussian_kl(g["mu"], g["mu0"], g["Sigma"], g["L"]) for g in self.latents)
        tot -= self.rho * augmented_kl(self.likelihood, self.local_vars, y, self.elbo_mode)
        tot -= self.extra_kl()
        return float(tot)

    def _as_svgp(self):
        helper = SVGP.__new__(SVGP)
        helper.likelihood, helper.jitter = self.likelihood, self.jitter
        helper.latents = []
        for g in self.latents:
            lt = Latent(g["kernel"], g["Z"])
            lt.mu, lt.Sigma, lt.K, lt.L = g["mu"], g["Sigma"], g["K"], g["L"]
            helper.latents.append(lt)
        return helper

    def predict_f(self, Xt, cov=False):
        return self._as_svgp().predict_f(Xt, cov)

    def predict_y(self, Xt):
        return self._as_svgp().predict_y(Xt)

    def proba_y(self, Xt):
        return self._as_svgp().proba_y(Xt)


def _first_array(lv):
    v = next(iter(lv.values()))
    return v[0] if isinstance(v, list) else v
