"""NumPy restatement of the reference GP with Analytic() inference (src/models/GP.jl, src/inference/analytic.jl), in both modes.

construct  GP(X, y, kernel; noise, opt_noise) runs train!(model, 1) (GP.jl:63)
step       analytic_updates (analytic.jl:36-51): Sigma = K + sigma2 I, alpha = Sigma \\ (y - mu0); with opt_noise one ADAM ascent step on
           log sigma2 with the gradient g sigma2, g = (alpha' alpha - tr Sigma^-1) / 2 (mode "reference": ||alpha||_2, G2)
train      train!(model, iterations) (training.jl:13-111): a new noise / kernel optimiser state per call; the hyper step when
           n_iter % atfrequency == 0, n_iter >= 3 and the iteration is not the last one -- d log p / d theta =
           tr((alpha alpha' - Sigma^-1) dK/dtheta) / 2 at the step's Sigma (mode "reference": nothing moves, G1); K is refreshed
           after a hyper step; at the end compute_Ks + post_step! rebuild Sigma and alpha with the final sigma2
log p      -(r' Sigma^-1 r + log det Sigma + N log 2 pi) / 2, r = y - mu0 (mode "reference": r = y, G3)  GP.jl:87-92
predict    mu* = K*n alpha, var* = k** + jitt - diag(K*n Sigma^-1 Kn*)  predictions.jl:6-23 ; proba_y adds sigma2
"""
import copy

import numpy as np
import scipy.linalg as sla

from oracle import agp_ref as R


class GPRef:
    def __init__(self, kernel, X, y, noise=1e-5, opt_noise=True, mu0=None, mode="corrected", jitter=1e-4, optimiser=None,
                 atfrequency=1, construct=True):
        self.kernel = copy.deepcopy(kernel)
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.N = len(self.y)
        self.sigma2 = float(noise)
        self.noise_opt = R.Adam(0.05) if opt_noise is True else (opt_noise or None)
        self.mu0 = np.zeros(self.N) if mu0 is None else np.broadcast_to(np.asarray(mu0, dtype=np.float64), (self.N,)).copy()
        self.mode, self.jitter = mode, jitter
        self.opt, self.atfrequency = optimiser, atfrequency
        self.n_iter = 0
        self.sigma2_trace = []
        self.logp_trace = []
        self.refresh_K()
        self.post()
        if construct:
            self.train(1)

    def refresh_K(self):
        """compute_Ks: kernelmatrix(k, X) + jitt I  (latentgp.jl:201-203)"""
        self.K = self.kernel.matrix(self.X) + self.jitter * np.eye(self.N)

    def post(self):
        """Sigma = K + sigma2 I, alpha = Sigma \\ (y - mu0), and log p of this Sigma"""
        self.Sigma = self.K + self.sigma2 * np.eye(self.N)
        self.L = np.linalg.cholesky(self.Sigma)
        self.r = self.y - self.mu0
        self.alpha = sla.cho_solve((self.L, True), self.r)
        self.Sinv = sla.cho_solve((self.L, True), np.eye(self.N))
        yq = self.r if self.mode == "corrected" else self.y
        quad = float(yq @ sla.cho_solve((self.L, True), yq))
        self.logp = -(quad + 2.0 * float(np.sum(np.log(np.diag(self.L)))) + self.N * np.log(2.0 * np.pi)) / 2.0

    def noise_grad(self):
        a2 = float(self.alpha @ self.alpha)
        return ((a2 if self.mode == "corrected" else np.sqrt(a2)) - float(np.trace(self.Sinv))) / 2.0

    def step(self):
        self.post()
        self.logp_trace.append(self.logp)
        if self.noise_opt is not None:
            g = self.noise_grad()
            self.nstate, d = self.noise_opt.apply(self.nstate, np.array([g * self.sigma2]))
            self.sigma2 = float(np.exp(np.log(self.sigma2) + d[0]))
        self.sigma2_trace.append(self.sigma2)
        return self

    def grad_K(self):
        """adjoint of K of log p: (alpha alpha' - Sigma^-1) / 2"""
        return 0.5 * (np.outer(self.alpha, self.alpha) - self.Sinv)

    def hyper_grad(self):
        """(d log p / d variance, d log p / d scales[D]) through K = variance * base(d2(s .* x, s .* x')) + jitt I (the backward form
        of tests/_vgp_ref.py with the oracle's dphi_dd2; SqExponential / Matern52 / Matern32, scalar or ARD scale)"""
        ker, X, G = self.kernel, self.X, self.grad_K()
        s = np.broadcast_to(np.asarray(ker.scale, dtype=np.float64), (X.shape[1],))
        d2 = np.zeros((self.N, self.N))
        for d in range(X.shape[1]):
            diff = s[d] * (X[:, d][:, None] - X[None, :, d])
            d2 += diff * diff
        GK = G * ker.sigma2 * R.dphi_dd2(ker.kind, d2)
        dvar = float(np.sum(G * ker.base_from_d2(d2)))
        dscale = np.array([2.0 * s[d] * np.sum(GK * (X[:, d][:, None] - X[None, :, d]) ** 2) for d in range(X.shape[1])])
        return dvar, dscale

    def hyper_step(self):
        """ADAM / Descent / Momentum ascent on the variance and scales in log space (autotuning_utils.jl:47-67)"""
        ker, opt = self.kernel, self.opt
        gv, gs = self.hyper_grad()
        v, sc = ker.sigma2, np.atleast_1d(np.asarray(ker.scale, dtype=np.float64))
        gs = np.array([np.sum(gs)]) if np.isscalar(ker.scale) else gs
        if ker.has_variance:
            self.hstate[0], dv = opt.apply(self.hstate[0], np.array([v * gv]))
            ker.sigma2 = float(np.exp(np.log(v) + dv[0]))
        if ker.has_transform:
            self.hstate[1], ds = opt.apply(self.hstate[1], sc * gs)
            new = np.exp(np.log(sc) + ds)
            ker.scale = float(new[0]) if np.isscalar(ker.scale) else new
        self.refresh_K()

    def train(self, iterations):
        """train!(model, iterations) without a state: new optimiser states, then compute_Ks + post_step! at the end"""
        if self.noise_opt is not None:
            self.nstate = self.noise_opt.init(np.zeros(1))
        if self.opt is not None:
            self.hstate = [self.opt.init(np.zeros(1)), self.opt.init(np.zeros(np.size(self.kernel.scale)))]
        for it in range(iterations):
            self.step()
            if (self.opt is not None and self.mode == "corrected" and self.n_iter % self.atfrequency == 0 and self.n_iter >= 3
                    and it + 1 != iterations):
                self.hyper_step()
            self.n_iter += 1
        self.refresh_K()
        self.post()
        return self

    def predict_f(self, Xt):
        Xt = np.asarray(Xt, dtype=np.float64)
        Ks = self.kernel.matrix(Xt, self.X)
        mu = Ks @ self.alpha
        var = self.kernel.diag(Xt) + self.jitter - np.einsum("ij,jk,ik->i", Ks, self.Sinv, Ks)
        cov = self.kernel.matrix(Xt) + self.jitter * np.eye(len(Xt)) - Ks @ self.Sinv @ Ks.T
        return mu, var, cov

    def proba_y(self, Xt):
        mu, var, _ = self.predict_f(Xt)
        return mu, var + self.sigma2
