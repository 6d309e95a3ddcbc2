"""NumPy restatement of MCIntegrationVI / MCIntegrationSVI for the SoftMax and LogisticSoftMax likelihoods (src/inference/MCVI.jl,
src/likelihood/softmax.jl, src/likelihood/logisticsoftmax.jl:144-193), written from the specification in include/agp_hip.h
("MC INTEGRATION"): the Monte-Carlo table from the Philox stream contract (streams 2 and 3, with log and cos by the stated arithmetic,
so the table is the device's bit for bit), the closed forms of log p and of its first two derivatives in their stable form, and the
K-fold step.  The optimiser rules, the positive-definiteness backtracking and the margins it records are those of the
single-latent restatement (tests/_nvi_ref.py): every latent is one NviRef that receives its gradients from here.
"""
import math

import numpy as np
import scipy.linalg as sla

import _nvi_ref as Q
from oracle import agp_ref as R

STREAM_GRAD, STREAM_ELBO = 2, 3
LINKS = ("softmax", "logisticsoftmax")
_U = np.uint64
_M32 = _U(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (the generator of tests/_mcgp_ref.py, vectorised)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = _U(k0), _U(k1)
    for _ in range(10):
        p0, p1 = _U(0xD2511F53) * c0, _U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> _U(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _U(0x9E3779B9)) & _M32, (k1 + _U(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def u53(hi, lo):
    return ((((hi >> _U(5)) << _U(26)) | (lo >> _U(6))).astype(np.float64) + 0.5) * 2.0 ** -53


def mc_log(a):
    """log a, 0 < a < 1, by the arithmetic of the contract (one IEEE operation per written operation)"""
    m, e = np.frexp(a)
    low = m < 0.7071067811865476
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e).astype(np.float64)
    q = (m - 1.0) / (m + 1.0)
    z = q * q
    p = np.full_like(z, 1.0 / 23.0)
    for d in range(21, 0, -2):
        p = p * z + 1.0 / d
    return e * 0.6931471805599453 + (2.0 * q) * p


def _fact(n):
    return float(math.factorial(n))


def mc_cos2pi(b):
    """cos(2 pi b), 0 < b < 1, by the arithmetic of the contract"""
    r = np.where(b > 0.5, 1.0 - b, b)
    flip = r > 0.25
    r = np.where(flip, 0.5 - r, r)
    sine = r > 0.125
    x = 6.283185307179586 * np.where(sine, 0.25 - r, r)
    z = x * x
    ps = np.full_like(z, 1.0 / _fact(17))
    for n, sg in ((15, -1), (13, 1), (11, -1), (9, 1), (7, -1), (5, 1), (3, -1)):
        ps = ps * z + sg * (1.0 / _fact(n))
    ps = x * (ps * z + 1.0)
    pc = np.full_like(z, 1.0 / _fact(16))
    for n, sg in ((14, -1), (12, 1), (10, -1), (8, 1), (6, -1), (4, 1), (2, -1)):
        pc = pc * z + sg * (1.0 / _fact(n))
    pc = pc * z + 1.0
    return np.where(flip, -1.0, 1.0) * np.where(sine, ps, pc)


def normals(seed, t, stream, nMC, K):
    """eps[nMC, K]: the Normal of block 0 at counter (s K + k, t, stream, 0), key = seed"""
    i = np.arange(nMC * K, dtype=np.uint64)
    one = np.ones_like(i)
    w = philox4x32_10(i, one * _U(t), one * _U(stream), one * _U(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    a, b = u53(w[0], w[1]), u53(w[2], w[3])
    return (np.sqrt(-2.0 * mc_log(a)) * mc_cos2pi(b)).reshape(nMC, K)


def terms(link, cls, f):
    """per draw: log p(c | f), d log p / d f_k, d2 log p / d f_k^2 for f [..., K] and the class index cls [...] (broadcast over the
    leading axes), in the stable form of the header: 1 - s of the largest entry is (sum of the others) / total"""
    f = np.asarray(f, dtype=np.float64)
    K = f.shape[-1]
    y = np.arange(K) == np.asarray(cls)[..., None]
    top = np.arange(K) == np.argmax(f, axis=-1)[..., None]  # (argmax: the first maximum)
    fc = np.sum(np.where(y, f, 0.0), axis=-1)
    if link == "softmax":
        M = np.max(f, axis=-1, keepdims=True)
        e = np.exp(f - M)
        Sp = np.sum(np.where(top, 0.0, e), axis=-1, keepdims=True)
        S = 1.0 + Sp
        sk = e / S
        om = np.where(top, Sp / S, 1.0 - sk)
        return (fc - M[..., 0]) - np.log1p(Sp[..., 0]), np.where(y, om, -sk), -sk * om
    if link == "logisticsoftmax":
        ex = np.exp(-np.abs(f))
        sg = np.where(f >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))
        sm = np.where(f >= 0, ex / (1.0 + ex), 1.0 / (1.0 + ex))
        Sp = np.sum(np.where(top, 0.0, sg), axis=-1, keepdims=True)
        St = np.sum(np.where(top, sg, 0.0), axis=-1, keepdims=True)
        S = St + Sp
        sk = sg / S
        om = np.where(top, Sp / S, 1.0 - sk)
        d = np.where(y, om, -sk)
        exc = np.exp(-np.abs(fc))
        logsg_c = np.where(fc >= 0, -np.log1p(exc), fc - np.log1p(exc))  # -softplus(-f_c)
        c_top = np.any(y & top, axis=-1)  # log s_c of the largest entry: -log1p(others / sg_c), no cancellation as s_c -> 1
        ell = np.where(c_top, -np.log1p(Sp[..., 0] / St[..., 0]), logsg_c - np.log(S[..., 0]))
        return ell, sm * d, sm * (-sg * d - sk * om * sm)
    raise ValueError(link)


def expectations(link, cls, mu, var, eps, chunk=64):
    """(ell [n], g [K, n], h [K, n], (|ell|, |g|, |h|) means of the absolute per-draw terms) for mu, var [K, n] and the table eps"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    K, n = mu.shape
    sd = np.sqrt(np.maximum(var, 0.0))
    out = [np.empty(n), np.empty((K, n)), np.empty((K, n)), np.empty(n), np.empty((K, n)), np.empty((K, n))]
    for a in range(0, n, chunk):
        s = slice(a, min(a + chunk, n))
        f = mu[:, s].T[:, None, :] + sd[:, s].T[:, None, :] * eps[None, :, :]  # [points, draws, K]
        L, G, H = terms(link, np.asarray(cls)[s][:, None], f)
        out[0][s], out[3][s] = L.mean(axis=1), np.abs(L).mean(axis=1)
        out[1][:, s], out[4][:, s] = G.mean(axis=1).T, np.abs(G).mean(axis=1).T
        out[2][:, s], out[5][:, s] = H.mean(axis=1).T, np.abs(H).mean(axis=1).T
    return out[0], out[1], out[2], tuple(out[3:])


def link_proba(link, mf):
    """the link at the mean (multiclass.jl:96-117): mf [K, n] -> p [n, K]"""
    mf = np.asarray(mf, dtype=np.float64).T
    if link == "softmax":
        e = np.exp(mf - mf.max(axis=1, keepdims=True))
    else:
        e = Q._sig(mf)
    return e / e.sum(axis=1, keepdims=True)


class McRef:
    """VGP(X, y, kernel, lik, MCIntegrationVI(nMC=nMC, optimiser=opt, natural=natural, seed=seed)): K latents on the training
    inputs, every one a single-latent NviRef (state, optimiser rule, backtracking, margins)"""

    def __init__(self, kernel, link, K, X, nMC, seed, make_opt, natural=True, jitter=1e-4):
        self.link, self.K, self.nMC, self.seed, self.natural = link, K, nMC, seed, natural
        self.lat = [Q.NviRef(kernel, None, X, n=1, opt=make_opt(), natural=natural, jitter=jitter) for _ in range(K)]
        self.t = 0
        self.alphas = []

    # the batch as the latents see it: (kappa or None, mean_f [K, B], var_f [K, B])
    def moments(self, Xb=None):
        return None, np.stack([r.mu for r in self.lat]), np.stack([np.diag(r.Sigma) for r in self.lat])

    def _latent_grads(self, r, kappa, g, h, rho):
        Sinv = np.linalg.inv(r.Sigma)
        if kappa is None:
            g2, g1 = np.diag(h / 2.0), g
        else:
            g2, g1 = R.rho_kappa_diag_theta_kappa(rho, kappa, h / 2.0), rho * kappa.T @ g
        g2 = g2 - (r.Kinv - Sinv) / 2.0
        g1 = g1 - sla.cho_solve((r.L, True), r.mu - r.mu0)
        if self.natural:
            g2 = 2.0 * r.Sigma @ g2 @ r.Sigma
            g1 = r.K @ g1
        return g1, g2

    def step(self, cls, Xb=None, rho=1.0):
        kappas, mf, vf = self.moments(Xb)
        eps = normals(self.seed, self.t + 1, STREAM_GRAD, self.nMC, self.K)
        _, g, h, _ = expectations(self.link, cls, mf, vf, eps)
        for k, r in enumerate(self.lat):
            r._grads_now = self._latent_grads(r, None if kappas is None else kappas[k], g[k], h[k], rho)
            Q.NviRef.step(r, None)
        self.t += 1
        self.alphas.append(tuple(r.alphas[-1] for r in self.lat))

    def elbo(self, cls, Xb=None, rho=1.0):
        _, mf, vf = self.moments(Xb)
        eps = normals(self.seed, self.t, STREAM_ELBO, self.nMC, self.K)
        ell, _, _, _ = expectations(self.link, cls, mf, vf, eps)
        return rho * float(np.sum(ell)) - sum(R.gaussian_kl(r.mu, r.mu0, r.Sigma, r.L) for r in self.lat)

    @property
    def margins(self):
        return [m for r in self.lat for m in r.margins]

    def counters(self):
        return [(r.halvings, r.rejected) for r in self.lat]


class McSparseRef(McRef):
    """SVGP(kernel, lik, MCIntegrationVI / MCIntegrationSVI, Z): the same on m inducing points; a step sees the minibatch through
    kappa = K_nm K^-1, K~ and rho = N / B"""

    def __init__(self, kernel, link, K, Z, nMC, seed, make_opt, natural=True, jitter=1e-4):
        super().__init__(kernel, link, K, Z, nMC, seed, make_opt, natural, jitter)
        self.lat = [Q.NviSparseRef(kernel, None, Z, n=1, opt=make_opt(), natural=natural, jitter=jitter) for _ in range(K)]

    def moments(self, Xb):
        ms = [r.moments(Xb) for r in self.lat]
        return [m[0] for m in ms], np.stack([m[1] for m in ms]), np.stack([m[2] for m in ms])

    def predict_f(self, Xt):
        ps = [r.predict_f(Xt) for r in self.lat]
        return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
