"""NumPy restatement of pathwise posterior sampling, written from the specification in include/agp_hip.h ("PATHWISE SAMPLING"):
the spectral draw and the Normal tables from the Philox stream contract (so Omega, the phases, W and E are the device's bit for
bit), and V and the paths from the formulas with NumPy's own cos, inv and cholesky.  The generator and the log / cos 2 pi
arithmetic are those of tests/_mcvi_ref.py.
"""
import math

import numpy as np

from _mcvi_ref import _U, mc_cos2pi, mc_log, philox4x32_10, u53

KINDS = ("sqexponential", "matern52", "matern32", "exponential")
NU = {"matern52": 2.5, "matern32": 1.5, "exponential": 0.5}
N_LOG = {"matern52": 2, "matern32": 1, "exponential": 0}  # K: exponentials on top of n^2 / 2 in the rejection-free Gamma(nu, 1)
Z, GAMMA, PHASE, W, E = range(5)  # stream offsets behind s0 = 4 + 8 latent


def _block(idx, t, stream, blk, seed):
    i = np.asarray(idx, dtype=np.uint64)
    one = np.ones_like(i)
    return philox4x32_10(i, one * _U(t), one * _U(stream), one * _U(blk), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def normal(idx, t, stream, seed):
    """the Normal of block 0 at counter (idx, t, stream, 0)"""
    w = _block(idx, t, stream, 0, seed)
    return np.sqrt(-2.0 * mc_log(u53(w[0], w[1]))) * mc_cos2pi(u53(w[2], w[3]))


def gamma_nu(kind, n_features, seed, t, latent=0):
    """G_j ~ Gamma(nu, 1), j < n_features, without rejection: n_j^2 / 2 minus K logarithms of uniforms"""
    s0 = 4 + 8 * latent
    j = np.arange(n_features)
    n = normal(j, t, s0 + GAMMA, seed)
    g = (n * n) * 0.5
    w = _block(j, t, s0 + GAMMA, 1, seed)
    for u in (u53(w[0], w[1]), u53(w[2], w[3]))[: N_LOG[kind]]:
        g = g - mc_log(u)
    return g


def features(kind, D, n_features, seed, t, latent=0):
    """(omega [l, D], phase [l]) of the contract"""
    s0 = 4 + 8 * latent
    om = normal(np.arange(n_features * D), t, s0 + Z, seed).reshape(n_features, D)
    if kind != "sqexponential":
        om = om * np.sqrt(NU[kind] / gamma_nu(kind, n_features, seed, t, latent))[:, None]
    w = _block(np.arange(n_features), t, s0 + PHASE, 0, seed)
    return om, 6.283185307179586 * u53(w[0], w[1])


def table(stream_off, rows, S, seed, t, latent=0):
    """W (stream_off = W, rows = l) or E (stream_off = E, rows = m): [rows, S], entry (r, s) at counter r S + s"""
    return normal(np.arange(rows * S), t, 4 + 8 * latent + stream_off, seed).reshape(rows, S)


def scales_of(scale, D):
    return np.full(D, float(scale)) if np.isscalar(scale) else np.asarray(scale, dtype=np.float64)


def kernel(kind, scale, sigma2, X, Y):
    """sigma2 k(||s o (x - y)||) for the four kernels"""
    s = scales_of(scale, X.shape[1])
    d2 = np.zeros((len(X), len(Y)))
    for d in range(X.shape[1]):
        diff = s[d] * X[:, d][:, None] - s[d] * Y[:, d][None, :]
        d2 += diff * diff
    if kind == "sqexponential":
        return sigma2 * np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if kind == "matern52":
        return sigma2 * (1.0 + math.sqrt(5.0) * r + 5.0 * d2 / 3.0) * np.exp(-math.sqrt(5.0) * r)
    if kind == "matern32":
        return sigma2 * (1.0 + math.sqrt(3.0) * r) * np.exp(-math.sqrt(3.0) * r)
    return sigma2 * np.exp(-r)


def phi(X, scale, sigma2, omega, phase):
    """Phi(X) [n, l]: sqrt(2 sigma2 / l) cos(omega_j' (s o x) + p_j)"""
    Xs = np.asarray(X, dtype=np.float64) * scales_of(scale, X.shape[1])
    return math.sqrt(2.0 * sigma2 / len(phase)) * np.cos(Xs @ omega.T + phase[None, :])


class Draw:
    """one latent's draw: the tables, V, and the paths as a function"""

    def __init__(self, kind, scale, sigma2, Zp, S, n_features, seed, t, latent=0):
        self.kind, self.scale, self.sigma2, self.Z = kind, scale, sigma2, np.asarray(Zp, dtype=np.float64)
        m, D = self.Z.shape
        self.omega, self.phase = features(kind, D, n_features, seed, t, latent)
        self.W = table(W, n_features, S, seed, t, latent)
        self.E = table(E, m, S, seed, t, latent)
        self.PhiZ = phi(self.Z, scale, sigma2, self.omega, self.phase)
        self.V = None

    def sparse(self, mu, eta2, jitter=1e-4):
        """SVGP / VGP: U = mu 1' + Xa' E, Xa = chol_lower(-2 eta2)^-1; V = K^-1 (U - Phi(Z) W)"""
        Xa = np.linalg.inv(np.linalg.cholesky(-2.0 * np.asarray(eta2)))
        self.U = np.asarray(mu)[:, None] + Xa.T @ self.E
        K = kernel(self.kind, self.scale, self.sigma2, self.Z, self.Z) + jitter * np.eye(len(self.Z))
        self.V = np.linalg.inv(K) @ (self.U - self.PhiZ @ self.W)
        return self

    def exact(self, alpha, Sigma_y, noise):
        """exact GP: V = alpha 1' - Sigma_y^-1 (Phi(X) W + sigma E), Sigma_y = K + noise I as the handle exports it"""
        self.V = np.asarray(alpha)[:, None] - np.linalg.inv(np.asarray(Sigma_y)) @ (self.PhiZ @ self.W + math.sqrt(noise) * self.E)
        return self

    def __call__(self, X):
        """[S, n_t]"""
        X = np.asarray(X, dtype=np.float64)
        F = phi(X, self.scale, self.sigma2, self.omega, self.phase) @ self.W
        return (F + kernel(self.kind, self.scale, self.sigma2, X, self.Z) @ self.V).T


def moments_sparse(d, X, mu, Sigma, jitter=1e-4):
    """mean and covariance of the paths at X given the features: k* K^-1 mu and G G' + k* K^-1 Sigma K^-1 k*'"""
    K = kernel(d.kind, d.scale, d.sigma2, d.Z, d.Z) + jitter * np.eye(len(d.Z))
    A = kernel(d.kind, d.scale, d.sigma2, X, d.Z) @ np.linalg.inv(K)
    G = phi(X, d.scale, d.sigma2, d.omega, d.phase) - A @ d.PhiZ
    return A @ mu, G @ G.T + A @ Sigma @ A.T


def moments_exact(d, X, alpha, Sigma_y, noise):
    """exact GP: k* alpha and G G' + noise k* Sigma_y^-2 k*', G = Phi(x) - k* Sigma_y^-1 Phi(X)"""
    ks = kernel(d.kind, d.scale, d.sigma2, X, d.Z)
    A = ks @ np.linalg.inv(Sigma_y)
    G = phi(X, d.scale, d.sigma2, d.omega, d.phase) - A @ d.PhiZ
    return ks @ alpha, G @ G.T + noise * A @ A.T
