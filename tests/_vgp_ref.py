"""NumPy restatement of the reference VGP with AnalyticVI (src/models/VGP.jl, kappa = I), built on the oracle's likelihood pieces.

step     update_parameters! (training.jl:140-144): local_updates! on mean_f = mu, var_f = diag Sigma (latentgp.jl:171-189), then
         natural_gradient!(::VarLatent) eta1 = grad_E_mu + K \\ mu0, eta2 = -(Diagonal(grad_E_Sigma) + inv(K)/2)
         (analyticVI.jl:126-140) and global_update! Sigma = -inv(eta2)/2, mu = Sigma eta1 (inference.jl:25-28)
elbo     analyticVI.jl:255-274 with rho = 1: expec_loglikelihood(mu, diag Sigma) - GaussianKL(mu, mu0, Sigma, K) - AugmentedKL
predict  the generic _predict_f with Zviews(m) = X (predictions.jl:25-50)
hyper    update_hyperparameters! (autotuning.jl:49-85): the gradient of -GaussianKL w.r.t. each latent's kernel variance and
         ScaleTransform / ARDTransform scales (SqExponential, Matern52, Matern32), ADAM ascent with the positive parameters stepped
         in log space (autotuning_utils.jl:47-67); every latent owns a deep copy of the kernel (latentgp.jl:34-36)
train    train!(model, iterations) (training.jl:13-120): step, then the hyper step when n_iter % atfrequency == 0, n_iter >= 3 and the
         iteration is not the last one; K is refreshed after a hyper step
"""
import copy

import numpy as np
import scipy.linalg as sla

from oracle import agp_ref as R


class VGPRef:
    def __init__(self, kernel, lik, X, jitter=1e-4, mu0=None):
        self.lik, self.X, self.jitter = lik, np.asarray(X, dtype=np.float64), jitter
        N = len(self.X)
        self.nl = lik.n_latent
        self.kernels = [copy.deepcopy(kernel) for _ in range(self.nl)]
        self.mu0 = [np.zeros(N) if mu0 is None else np.asarray(mu0, float).copy() for _ in range(self.nl)]
        self.mu = [np.zeros(N) for _ in range(self.nl)]  # VarPosterior init (posterior.jl:29-37)
        self.Sigma = [np.eye(N) for _ in range(self.nl)]
        self.eta1 = [np.zeros(N) for _ in range(self.nl)]
        self.eta2 = [-0.5 * np.eye(N) for _ in range(self.nl)]
        self.lv = None
        self.refresh_K()

    @property
    def kernel(self):
        """latent 0's kernel"""
        return self.kernels[0]

    @property
    def K(self):
        return self.Ks[0]

    @property
    def L(self):
        return self.Ls[0]

    @property
    def Kinv(self):
        return self.Kinvs[0]

    def refresh_K(self):
        """compute_K(gp, X, jitt): cholesky(kernelmatrix(k, X) + jitt I) per latent  latentgp.jl:201-203"""
        self.Ks, self.Ls, self.Kinvs = [], [], []
        for ker in self.kernels:
            K, L = R.compute_K(ker, self.X, self.jitter)
            Kinv = sla.cho_solve((L, True), np.eye(len(self.X)))
            self.Ks.append(K)
            self.Ls.append(L)
            self.Kinvs.append((Kinv + Kinv.T) / 2.0)

    def mean_f(self):
        return tuple(self.mu)

    def var_f(self):
        return tuple(np.diag(S).copy() for S in self.Sigma)

    def step(self, y):
        if self.lv is None:
            self.lv = R.init_local_vars(self.lik, len(y))
        self.lv = R.local_updates(self.lv, self.lik, y, self.mean_f(), self.var_f())
        g1 = R.grad_E_mu(self.lik, y, self.lv)
        g2 = R.grad_E_Sigma(self.lik, y, self.lv)
        for k in range(self.nl):
            self.eta1[k] = g1[k] + sla.cho_solve((self.Ls[k], True), self.mu0[k])
            self.eta2[k] = -(np.diag(g2[k]) + self.Kinvs[k] / 2.0)
            self.mu[k], self.Sigma[k] = R.natural_to_standard(self.eta1[k], self.eta2[k])
        return self

    def elbo(self, y, mode="corrected"):
        e = R.expec_loglikelihood(self.lik, y, self.mean_f(), self.var_f(), self.lv, mode)
        kl = sum(R.gaussian_kl(self.mu[k], self.mu0[k], self.Sigma[k], self.Ls[k]) for k in range(self.nl))
        return e - kl - R.augmented_kl(self.lik, self.lv, y, mode)

    def elbo_fresh(self, y):
        """ELBO(model) on the training set with fresh local variables (ELBO.jl:28-47)"""
        lv = R.init_local_vars(self.lik, len(y))
        saved, self.lv = self.lv, R.local_updates(lv, self.lik, y, self.mean_f(), self.var_f())
        out = self.elbo(y)
        self.lv = saved
        return out

    def predict_f(self, Xt):
        """mu* = K*n K^-1 mu ; var* = k** + jitt - diag(K*n A Kn*), A = K^-1 - K^-1 Sigma K^-1  (predictions.jl:25-50)"""
        Xt = np.asarray(Xt, float)
        mus, vars_, covs = [], [], []
        for k in range(self.nl):
            ker, Kinv = self.kernels[k], self.Kinvs[k]
            Ks = ker.matrix(Xt, self.X)
            kss = ker.diag(Xt) + self.jitter
            a = Kinv @ self.mu[k]
            A = Kinv - Kinv @ self.Sigma[k] @ Kinv
            mus.append(Ks @ a)
            vars_.append(kss - np.einsum("ij,jk,ik->i", Ks, A, Ks))
            covs.append(ker.matrix(Xt) + self.jitter * np.eye(len(Xt)) - Ks @ A @ Ks.T)
        return mus, vars_, covs

    def hyper_grad(self, k=0):
        """(d ELBO / d variance, d ELBO / d scales[D]) of latent k through K = variance * base(d2(s .* x, s .* x')) + jitt I, with
        G_K = kl_grad_K(k): the backward form of the oracle's hyper_gradient_core (back(G_K, X, X)) with its dphi_dd2, so
        SqExponential / Matern52 / Matern32 and a scalar or ARD scale.  For a ScaleTransform the scale's gradient is the sum."""
        ker, X = self.kernels[k], self.X
        G = self.kl_grad_K(k)
        s = np.broadcast_to(np.asarray(ker.scale, dtype=np.float64), (X.shape[1],))
        d2 = np.zeros((len(X), len(X)))
        for d in range(X.shape[1]):
            diff = s[d] * (X[:, d][:, None] - X[None, :, d])
            d2 += diff * diff
        GK = G * ker.sigma2 * R.dphi_dd2(ker.kind, d2)  # dL / dd2
        dvar = float(np.sum(G * ker.base_from_d2(d2)))
        dscale = np.array([2.0 * s[d] * np.sum(GK * (X[:, d][:, None] - X[None, :, d]) ** 2) for d in range(X.shape[1])])
        return dvar, dscale

    def hyper_step(self, opt):
        """ADAM ascent on every latent's variance and scales in log space; one optimiser state per parameter (per scale dimension
        for an ARDTransform)"""
        if getattr(self, "hstate", None) is None:
            self.hstate = [[opt.init(np.zeros(1)), opt.init(np.zeros(np.size(ker.scale)))] for ker in self.kernels]
        for k, ker in enumerate(self.kernels):
            gv, gs = self.hyper_grad(k)
            v, sc = ker.sigma2, np.atleast_1d(np.asarray(ker.scale, dtype=np.float64))
            gs = np.array([np.sum(gs)]) if np.isscalar(ker.scale) else gs
            if ker.has_variance:
                self.hstate[k][0], dv = opt.apply(self.hstate[k][0], np.array([v * gv]))
                ker.sigma2 = float(np.exp(np.log(v) + dv[0]))
            if ker.has_transform:
                self.hstate[k][1], ds = opt.apply(self.hstate[k][1], sc * gs)
                new = np.exp(np.log(sc) + ds)
                ker.scale = float(new[0]) if np.isscalar(ker.scale) else new
        self.refresh_K()

    def train(self, y, iterations, opt=None, atfrequency=1, callback=None):
        n_iter = getattr(self, "n_iter", 0)
        for it in range(iterations):
            self.step(y)
            if callback is not None:
                callback(self)
            if opt is not None and n_iter % atfrequency == 0 and n_iter >= 3 and it + 1 != iterations:
                self.hyper_step(opt)
            n_iter += 1
        self.n_iter = n_iter
        return self

    def kl_grad_K(self, k=0):
        """adjoint of K of -GaussianKL: (K^-1 (Sigma + d d') K^-1 - K^-1) / 2, d = mu - mu0  (autotuning.jl:49-85)"""
        Kinv = self.Kinvs[k]
        Kd = Kinv @ (self.mu[k] - self.mu0[k])
        return 0.5 * (Kinv @ self.Sigma[k] @ Kinv + np.outer(Kd, Kd) - Kinv)
