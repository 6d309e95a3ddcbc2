"""NumPy restatement of QuadratureVI on the full and the sparse model (src/inference/numericalVI.jl, src/inference/quadratureVI.jl), written from the
reference's formulas AS THEY STAND there -- inv(K), inv(Sigma), 2 Sigma grad Sigma -- not from the device's inverse-free form, with
the three definitions the device restates (include/agp_hip.h, "NUMERICAL INFERENCE"): Logistic l'', Laplace E[l''], no clipping.

Kernels, the Gaussian KL and the optimiser rules are the oracle's (oracle/agp_ref.py).  Every positive-definiteness decision of the
backtracking records |lambda_min| / lambda_max of the matrix it judged (NviRef.margins), and the Laplace nodes their distance from
the kink: the margin condition under which host and device must take the same decisions.
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle import agp_ref as R


def gh_rule(n):
    """x_j = sqrt(2) t_j, w_j = omega_j / sqrt(pi)   (quadratureVI.jl:36-40)"""
    t, om = np.polynomial.hermite.hermgauss(int(n))
    return np.ascontiguousarray(t * math.sqrt(2.0)), np.ascontiguousarray(om / math.sqrt(math.pi))


def _sig(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loglik(lik, y, f):
    """l(y, f), elementwise (y broadcast against f)"""
    if lik.name == "logistic":  # -log(1 + exp(-y f)), overflow-safe on both sides
        z = -y * f
        return np.where(z > 0, -(z + np.log1p(np.exp(-np.abs(z)))), -np.log1p(np.exp(-np.abs(z))))
    if lik.name == "studentt":  # the density as written, studentt.jl:43-46
        a = lik.alpha
        c = math.lgamma(a) - 0.5 * math.log(lik.nu * math.pi) - math.lgamma(lik.nu / 2.0)
        u = (y - f) / lik.sigma
        return c - a * np.log(1.0 + u * u)
    if lik.name == "laplace":
        return -np.abs(y - f) / lik.beta - math.log(2.0 * lik.beta)
    raise ValueError(lik.name)


def dloglik(lik, y, f):
    if lik.name == "logistic":
        return y * _sig(-y * f)
    if lik.name == "studentt":
        u = (y - f) / lik.sigma
        return 2.0 * lik.alpha * u / (lik.sigma * (1.0 + u * u))
    if lik.name == "laplace":
        return np.sign(y - f) / lik.beta
    raise ValueError(lik.name)


def d2loglik(lik, y, f):
    if lik.name == "logistic":
        return -_sig(f) * _sig(-f) + 0.0 * y
    if lik.name == "studentt":
        u = (y - f) / lik.sigma
        return -2.0 * lik.alpha * (1.0 - u * u) / (lik.sigma ** 2 * (1.0 + u * u) ** 2)
    raise ValueError(lik.name)


def expectations(lik, y, mu, var, x, w):
    """(ell, g, h, termsum): per point sum_j w_j l, sum_j w_j l', sum_j w_j l'' (Laplace: the closed form) and, for error bounds,
    sum_j w_j |term_j| of each of the three."""
    y, mu, var = (np.asarray(a, dtype=np.float64) for a in (y, mu, var))
    f = mu[:, None] + np.sqrt(np.maximum(var, 0.0))[:, None] * x[None, :]
    yy = y[:, None]
    L, G = loglik(lik, yy, f), dloglik(lik, yy, f)
    ell, g = L @ w, G @ w
    if lik.name == "laplace":
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(var > 0, -(2.0 / lik.beta) * np.exp(-0.5 * (y - mu) ** 2 / var) / np.sqrt(2.0 * math.pi * var), 0.0)
        habs = np.abs(h)
    else:
        H = d2loglik(lik, yy, f)
        h, habs = H @ w, np.abs(H) @ w
    return ell, g, h, (np.abs(L) @ w, np.abs(G) @ w, habs)


def laplace_node_margin(y, mu, var, x):
    """min over points and nodes of |y_i - f_ij| / (|y_i| + |f_ij| + 1): how far the quadrature stays from the kink of |y - f|"""
    f = mu[:, None] + np.sqrt(np.maximum(var, 0.0))[:, None] * x[None, :]
    return float(np.min(np.abs(y[:, None] - f) / (np.abs(y[:, None]) + np.abs(f) + 1.0)))


def make_rule(kind, eta, **kw):
    return {"descent": lambda: R.Descent(eta), "momentum": lambda: R.Momentum(eta, kw.get("rho", 0.9)),
            "adam": lambda: R.Adam(eta)}[kind]()


class NviRef:
    """VGP(X, y, kernel, lik, QuadratureVI(nGaussHermite=n, optimiser=opt, natural=natural)) for one latent"""

    def __init__(self, kernel, lik, X, n=100, opt=None, natural=True, mu0=None, jitter=1e-4):
        self.kernel, self.lik, self.X = kernel, lik, np.asarray(X, dtype=np.float64)
        N = len(self.X)
        self.N, self.jitter, self.natural = N, jitter, natural
        self.x, self.w = gh_rule(n)
        self.K = kernel.matrix(self.X) + jitter * np.eye(N)
        self.L = np.linalg.cholesky(self.K)
        self.Kinv = sla.cho_solve((self.L, True), np.eye(N))
        self.mu0 = np.zeros(N) if mu0 is None else np.asarray(mu0, dtype=np.float64)
        self.mu, self.Sigma = np.zeros(N), np.eye(N)
        self.opt = opt if opt is not None else R.Momentum(1e-5, 0.9)
        self.st_mu, self.st_S = self.opt.init(self.mu), self.opt.init(self.Sigma)
        self.alphas, self.halvings, self.rejected = [], 0, 0
        self.margins = []        # |lambda_min| / lambda_max of every matrix whose positive definiteness was decided
        self.node_margins = []   # Laplace: laplace_node_margin of every step

    def grads(self, y):
        """(grad_eta1, grad_eta2) as the optimiser receives them (numericalVI.jl:121-156)"""
        var = np.diag(self.Sigma).copy()
        _, g, h, _ = expectations(self.lik, y, self.mu, var, self.x, self.w)
        if self.lik.name == "laplace":
            self.node_margins.append(laplace_node_margin(y, self.mu, var, self.x))
        Sinv = np.linalg.inv(self.Sigma)
        g2 = np.diag(h / 2.0) - (self.Kinv - Sinv) / 2.0
        g1 = g - sla.cho_solve((self.L, True), self.mu - self.mu0)
        if self.natural:
            g2 = 2.0 * self.Sigma @ g2 @ self.Sigma
            g1 = self.K @ g1
        return g1, g2

    def step(self, y):
        g1, g2 = self.grads(y) if y is not None else self._grads_now  # (None: the sparse model has formed them on its batch)
        self.st_mu, dmu = self.opt.apply(self.st_mu, g1)
        self.st_S, dS = self.opt.apply(self.st_S, g2)
        self.mu = self.mu + dmu
        dS = np.triu(dS) + np.triu(dS, 1).T  # Symmetric(dSigma): the upper triangle
        a = 1.0
        while True:
            C = self.Sigma + a * dS
            ev = np.linalg.eigvalsh(C)
            self.margins.append(abs(ev[0]) / ev[-1])
            if ev[0] > 0 or not a > 1e-8:
                break
            a *= 0.5
            self.halvings += 1
        if a > 1e-8:
            self.Sigma = C
        else:
            self.rejected += 1
        self.alphas.append(a)

    def elbo(self, y):
        ell, _, _, _ = expectations(self.lik, y, self.mu, np.diag(self.Sigma), self.x, self.w)
        return float(np.sum(ell)) - R.gaussian_kl(self.mu, self.mu0, self.Sigma, self.L)

    def residuals(self, y):
        """relative residuals of the Opper-Archambeau fixed point mu - mu0 = K g, Sigma^-1 = K^-1 - Diagonal(h)"""
        _, g, h, _ = expectations(self.lik, y, self.mu, np.diag(self.Sigma), self.x, self.w)
        return fixed_point_residuals(self.K, self.mu0, self.mu, self.Sigma, g, h)

    def predict_f(self, Xt):
        """mu* = K*n K^-1 mu ; var* = k** + jitt - diag(K*n A Kn*), A = K^-1 - K^-1 Sigma K^-1  (predictions.jl:25-50)"""
        Ks = self.kernel.matrix(np.asarray(Xt, dtype=np.float64), self.X)
        A = self.Kinv - self.Kinv @ self.Sigma @ self.Kinv
        return Ks @ (self.Kinv @ self.mu), self.kernel.diag(Xt) + self.jitter - np.einsum("ij,jk,ik->i", Ks, A, Ks)


class NviSparseRef(NviRef):
    """SVGP(kernel, lik, QuadratureVI / QuadratureSVI, Z): the same state and optimiser on the m inducing points Z; a step sees
    the minibatch (X[idx], y[idx]) through kappa = K_nm K^-1, K~ and rho = N / B (numericalVI.jl:136-150, latentgp.jl:171-212)"""

    def __init__(self, kernel, lik, Z, **kw):
        super().__init__(kernel, lik, Z, **kw)
        self.Z = self.X

    def moments(self, Xb):
        Knm, kappa, Kt = R.compute_kappa(self.kernel, Xb, self.Z, self.L, self.jitter)
        return kappa, R.mean_f(self.mu, kappa), R.var_f(self.Sigma, kappa, Kt)

    def grads(self, Xb, yb, rho):
        kappa, mf, vf = self.moments(Xb)
        _, g, h, _ = expectations(self.lik, yb, mf, vf, self.x, self.w)
        if self.lik.name == "laplace":
            self.node_margins.append(laplace_node_margin(yb, mf, vf, self.x))
        Sinv = np.linalg.inv(self.Sigma)
        g2 = R.rho_kappa_diag_theta_kappa(rho, kappa, h / 2.0) - (self.Kinv - Sinv) / 2.0
        g1 = rho * kappa.T @ g - sla.cho_solve((self.L, True), self.mu - self.mu0)
        if self.natural:
            g2 = 2.0 * self.Sigma @ g2 @ self.Sigma
            g1 = self.K @ g1
        return g1, g2

    def step(self, Xb, yb, rho):
        self._grads_now = self.grads(Xb, yb, rho)
        NviRef.step(self, None)

    def elbo(self, Xb, yb, rho):
        _, mf, vf = self.moments(Xb)
        ell, _, _, _ = expectations(self.lik, yb, mf, vf, self.x, self.w)
        return rho * float(np.sum(ell)) - R.gaussian_kl(self.mu, self.mu0, self.Sigma, self.L)

    def predict_f(self, Xt):
        Ks = self.kernel.matrix(np.asarray(Xt, dtype=np.float64), self.Z)
        A = self.Kinv - self.Kinv @ self.Sigma @ self.Kinv
        return Ks @ (self.Kinv @ self.mu), self.kernel.diag(Xt) + self.jitter - np.einsum("ij,jk,ik->i", Ks, A, Ks)


def fixed_point_residuals(K, mu0, mu, Sigma, g, h):
    r1 = np.max(np.abs(mu - mu0 - K @ g)) / max(np.max(np.abs(mu - mu0)), 1e-300)
    P = np.linalg.inv(K) - np.diag(h)
    r2 = np.max(np.abs(np.linalg.inv(Sigma) - P)) / np.max(np.abs(P))
    return float(r1), float(r2)
