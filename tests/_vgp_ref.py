"""NumPy restatement of the reference VGP with AnalyticVI (src/models/VGP.jl, kappa = I), built on the oracle's likelihood pieces.

step     update_parameters! (training.jl:140-144): local_updates! on mean_f = mu, var_f = diag Sigma (latentgp.jl:171-189), then
         natural_gradient!(::VarLatent) eta1 = grad_E_mu + K \\ mu0, eta2 = -(Diagonal(grad_E_Sigma) + inv(K)/2)
         (analyticVI.jl:126-140) and global_update! Sigma = -inv(eta2)/2, mu = Sigma eta1 (inference.jl:25-28)
elbo     analyticVI.jl:255-274 with rho = 1: expec_loglikelihood(mu, diag Sigma) - GaussianKL(mu, mu0, Sigma, K) - AugmentedKL
predict  the generic _predict_f with Zviews(m) = X (predictions.jl:25-50)
hyper    update_hyperparameters! (autotuning.jl:49-85): the gradient of -GaussianKL w.r.t. the kernel's variance and ScaleTransform
         scale (SqExponentialKernel), ADAM ascent with the positive parameters stepped in log space (autotuning_utils.jl:47-67)
train    train!(model, iterations) (training.jl:13-120): step, then the hyper step when n_iter % atfrequency == 0, n_iter >= 3 and the
         iteration is not the last one; K is refreshed after a hyper step
"""
import numpy as np
import scipy.linalg as sla

from oracle import agp_ref as R


class VGPRef:
    def __init__(self, kernel, lik, X, jitter=1e-4, mu0=None):
        self.kernel, self.lik, self.X, self.jitter = kernel, lik, np.asarray(X, dtype=np.float64), jitter
        N = len(self.X)
        self.nl = lik.n_latent
        self.mu0 = [np.zeros(N) if mu0 is None else np.asarray(mu0, float).copy() for _ in range(self.nl)]
        self.mu = [np.zeros(N) for _ in range(self.nl)]  # VarPosterior init (posterior.jl:29-37)
        self.Sigma = [np.eye(N) for _ in range(self.nl)]
        self.eta1 = [np.zeros(N) for _ in range(self.nl)]
        self.eta2 = [-0.5 * np.eye(N) for _ in range(self.nl)]
        self.lv = None
        self.refresh_K()

    def refresh_K(self):
        """compute_K(gp, X, jitt): cholesky(kernelmatrix(k, X) + jitt I)  latentgp.jl:201-203"""
        self.K, self.L = R.compute_K(self.kernel, self.X, self.jitter)
        Kinv = sla.cho_solve((self.L, True), np.eye(len(self.X)))
        self.Kinv = (Kinv + Kinv.T) / 2.0

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
            self.eta1[k] = g1[k] + sla.cho_solve((self.L, True), self.mu0[k])
            self.eta2[k] = -(np.diag(g2[k]) + self.Kinv / 2.0)
            self.mu[k], self.Sigma[k] = R.natural_to_standard(self.eta1[k], self.eta2[k])
        return self

    def elbo(self, y, mode="corrected"):
        e = R.expec_loglikelihood(self.lik, y, self.mean_f(), self.var_f(), self.lv, mode)
        kl = sum(R.gaussian_kl(self.mu[k], self.mu0[k], self.Sigma[k], self.L) for k in range(self.nl))
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
        Ks = self.kernel.matrix(np.asarray(Xt, float), self.X)
        kss = self.kernel.diag(np.asarray(Xt, float)) + self.jitter
        mus, vars_, covs = [], [], []
        for k in range(self.nl):
            a = self.Kinv @ self.mu[k]
            A = self.Kinv - self.Kinv @ self.Sigma[k] @ self.Kinv
            mus.append(Ks @ a)
            vars_.append(kss - np.einsum("ij,jk,ik->i", Ks, A, Ks))
            covs.append(self.kernel.matrix(np.asarray(Xt, float)) + self.jitter * np.eye(len(Xt)) - Ks @ A @ Ks.T)
        return mus, vars_, covs

    def hyper_grad(self, k=0):
        """(d ELBO / d variance, d ELBO / d scale) through K = variance * exp(-scale^2 d2 / 2) + jitt I (SqExponentialKernel)"""
        assert self.kernel.kind == "sqexponential" and np.isscalar(self.kernel.scale)
        G = self.kl_grad_K(k)
        Kb = self.K - self.jitter * np.eye(len(self.X))  # variance * base
        X = self.X
        d2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)
        dvar = float(np.sum(G * Kb) / self.kernel.sigma2)
        dscale = float(np.sum(G * Kb * (-self.kernel.scale * d2)))
        return dvar, dscale

    def hyper_step(self, opt):
        if getattr(self, "hstate", None) is None:
            self.hstate = [opt.init(np.zeros(1)), opt.init(np.zeros(1))]
        gv, gs = self.hyper_grad(0)
        v, sc = self.kernel.sigma2, self.kernel.scale
        self.hstate[0], dv = opt.apply(self.hstate[0], np.array([v * gv]))
        self.hstate[1], ds = opt.apply(self.hstate[1], np.array([sc * gs]))
        self.kernel.sigma2 = float(np.exp(np.log(v) + dv[0]))
        self.kernel.scale = float(np.exp(np.log(sc) + ds[0]))
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
        d = self.mu[k] - self.mu0[k]
        Kd = self.Kinv @ d
        return 0.5 * (self.Kinv @ self.Sigma[k] @ self.Kinv + np.outer(Kd, Kd) - self.Kinv)
