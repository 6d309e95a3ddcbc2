"""NumPy / SciPy restatement of MCGP with GibbsSampling (src/models/MCGP.jl, src/inference/gibbssampling.jl,
src/training/sampling.jl, src/training/predictions.jl:94-130,260-276), transcribed from the specification in include/agp_hip.h
("Gibbs sampling", "RANDOM STREAMS"): Philox4x32-10, the stream contract, the three variate samplers, sample_local! /
sample_global! with the oracle's grad_E_mu / grad_E_Sigma and dense inv / cholesky, _predict_f / proba_y in their intended form.

Every data-dependent comparison -- accept / reject, and the two that choose a branch (1 / z > T in the truncated inverse Gaussian,
x > T in a(n, x)) -- goes through `gt`, which records the relative margin |a - b| / max(|a|, |b|) in MARGINS: the GPU
parity tests are only meaningful for inputs whose smallest margin is far above the difference between host and device arithmetic
(tests/test_mcgp_host.py asserts it for the parity cases).
"""
import math

import numpy as np
import scipy.linalg as sla
from scipy.special import erfc, erfcx

from oracle import agp_ref as R

MASK = 0xFFFFFFFF
PG_T = 0.64
MARGINS = []


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def u53(hi, lo):
    return ((((hi >> 5) << 26) | (lo >> 6)) + 0.5) * 2.0 ** -53


def gt(a, b):
    """a > b, with the relative margin of the comparison recorded (an infinite operand: margin 1)"""
    MARGINS.append(1.0 if math.isinf(a) or math.isinf(b) else abs(a - b) / max(abs(a), abs(b), 1e-300))
    return a > b


class Stream:
    """u_0, u_1, ... of (seed, t, stream, i): block j = Philox(ctr = (i, t, stream, j), key = (seed lo, seed hi)) gives u_2j, u_2j+1"""

    def __init__(self, seed, t, stream, i):
        self.key = (seed & MASK, (seed >> 32) & MASK)
        self.i, self.t, self.stream, self.j, self.held = i, t, stream, 0, None

    def u(self):
        if self.held is not None:
            v, self.held = self.held, None
            return v
        w = philox4x32_10((self.i, self.t, self.stream, self.j), self.key)
        self.j += 1
        self.held = u53(w[2], w[3])
        return u53(w[0], w[1])

    def expo(self):
        return -math.log(self.u())

    def normal(self):
        a = self.u()
        b = self.u()
        return math.sqrt(-2.0 * math.log(a)) * math.cos(6.283185307179586 * b)


def log_ndtr(x):
    s = x * 0.7071067811865476
    return math.log(0.5 * erfcx(-s)) - s * s if x < 0.0 else math.log1p(-0.5 * erfc(s))


def mass_texpon(z):
    K = math.pi ** 2 / 8 + 0.5 * z * z
    b, a = 1.25 * (PG_T * z - 1.0), -1.25 * (PG_T * z + 1.0)
    x0 = math.log(K) + K * PG_T
    return 1.0 / (1.0 + 4.0 / math.pi * (math.exp(x0 - z + log_ndtr(b)) + math.exp(x0 + z + log_ndtr(a))))


def a_coef(n, x):
    h = n + 0.5
    k = h * math.pi
    if gt(x, PG_T):
        return k * math.exp(-0.5 * k * k * x)
    return math.exp(-1.5 * (math.log(math.pi / 2) + math.log(x)) + math.log(k) - 2.0 * h * h / x)


def tig(s, z):
    mu = 1.0 / z if z > 0 else math.inf
    if gt(mu, PG_T):
        while True:
            while True:
                E, E2 = s.expo(), s.expo()
                if not gt(E * E, 2.0 * E2 / PG_T):
                    break
            x = PG_T / (1.0 + E * PG_T) ** 2
            if not gt(s.u(), math.exp(-0.5 * z * z * x)):
                return x
    while True:
        n = s.normal()
        w = mu * n * n
        x = mu + 0.5 * mu * w - 0.5 * mu * math.sqrt(4.0 * w + w * w)
        if gt(s.u(), mu / (mu + x)):
            x = mu * mu / x
        if not gt(x, PG_T):
            return x


def pg1(s, z, r):
    K = math.pi ** 2 / 8 + 0.5 * z * z
    while True:
        if gt(r, s.u()):
            x = PG_T + s.expo() / K
        else:
            x = tig(s, z)
        S = a_coef(0, x)
        y = s.u() * S
        n = 0
        while True:
            n += 1
            if n % 2:
                S -= a_coef(n, x)
                if not gt(y, S):
                    return 0.25 * x
            else:
                S += a_coef(n, x)
                if gt(y, S):
                    break


def pg(s, b, c):
    """PG(b, c), integer b: the sum of b draws of PG(1, c) from one stream"""
    z = 0.5 * abs(c)
    r = mass_texpon(z)
    return sum(pg1(s, z, r) for _ in range(int(b)))


def gamma_mt(s, alpha):
    a1 = alpha + 1.0 if alpha < 1.0 else alpha
    d = a1 - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    while True:
        z = s.normal()
        v1 = 1.0 + c * z
        if not gt(v1, 0.0):
            continue
        v = v1 * v1 * v1
        u = s.u()
        z2 = z * z
        if gt(1.0 - 0.0331 * z2 * z2, u):
            break
        if gt(0.5 * z2 + d * (1.0 - v + math.log(v)), math.log(u)):
            break
    g = d * v
    if alpha < 1.0:
        g *= math.exp(math.log(s.u()) / alpha)
    return g


def inverse_gamma(s, alpha, beta):
    return beta / gamma_mt(s, alpha)


def sample_local(lik, y, f, seed, t):
    """sample_local! (logistic.jl:53-60, studentt.jl:84-92, negativebinomial.jl:83-90) -> (theta, aux)"""
    n = len(f)
    theta, aux = np.zeros(n), np.zeros(n)
    for i in range(n):
        s = Stream(seed, t, 0, i)
        if lik.name == "studentt":
            aux[i] = inverse_gamma(s, 0.5 * (lik.nu + 1.0), 0.5 * ((f[i] - y[i]) ** 2 + lik.sigma ** 2 * lik.nu))
            theta[i] = 1.0 / aux[i]
        else:
            b = 1 if lik.name == "logistic" else int(y[i]) + int(lik.r)
            aux[i] = abs(f[i])
            theta[i] = pg(s, b, aux[i])
    return theta, aux


def normals(n, seed, t):
    return np.array([Stream(seed, t, 1, i).normal() for i in range(n)])


def kept_sweeps(n, discard_initial, thinning):
    return [discard_initial + 1 + k * thinning for k in range(n)]


class MCGPRef:
    def __init__(self, kernel, lik, X, y, seed, jitter=1e-4, mu0=None):
        self.kernel, self.lik, self.X, self.y = kernel, lik, np.asarray(X, float), np.asarray(y, float)
        self.seed, self.jitter = int(seed), jitter
        N = len(self.X)
        self.mu0 = np.zeros(N) if mu0 is None else np.asarray(mu0, float).copy()
        self.f = np.zeros(N)  # latentgp.jl:81-86
        self.Sigma = np.eye(N)
        self.theta = np.zeros(N)
        self.t = 0
        self.K, self.L = R.compute_K(kernel, self.X, jitter)
        Kinv = sla.cho_solve((self.L, True), np.eye(N))
        self.Kinv = (Kinv + Kinv.T) / 2.0
        self.kinv_mu0 = sla.cho_solve((self.L, True), self.mu0)

    def sweep(self):
        """one AbstractMCMC.step (sampling.jl:36-75): sample_local!, then sample_global! (gibbssampling.jl:50-60)"""
        self.theta, aux = sample_local(self.lik, self.y, self.f, self.seed, self.t)
        lv = {"theta": self.theta, "c": aux}
        g1 = R.grad_E_mu(self.lik, self.y, lv)[0]
        g2 = R.grad_E_Sigma(self.lik, self.y, lv)[0]
        A = 2.0 * np.diag(g2) + self.Kinv
        Xa = sla.solve_triangular(np.linalg.cholesky(A), np.eye(len(A)), lower=True)
        self.Sigma = Xa.T @ Xa
        eta1 = g1 + self.kinv_mu0
        self.f = Xa.T @ (Xa @ eta1 + normals(len(A), self.seed, self.t))  # ~ N(Sigma eta1, Sigma)
        self.t += 1
        return self.f

    def sample(self, n, discard_initial=0, thinning=1, trace=None):
        keep = set(kept_sweeps(n, discard_initial, thinning))
        out = []
        for s in range(1, max(keep) + 1):
            f = self.sweep()
            if trace is not None:
                trace.append(f.copy())
            if s in keep:
                out.append(f.copy())
        return np.array(out)

    # ---- predictions.jl:94-130, 260-276 in their intended form (DESIGN.md section 9h names the two defects) ---------------------
    def f_star(self, Xt, store):
        Ks = self.kernel.matrix(np.asarray(Xt, float), self.X)
        return (Ks @ self.Kinv) @ np.asarray(store).T, Ks  # (n_t, S)

    def predict_f(self, Xt, store):
        F, Ks = self.f_star(Xt, store)
        kss = self.kernel.diag(np.asarray(Xt, float)) + self.jitter
        return F.mean(axis=1), kss - np.einsum("ij,jk,ik->i", Ks, self.Kinv, Ks) + F.var(axis=1, ddof=1)

    def proba_y_logistic(self, Xt, store):
        F, _ = self.f_star(Xt, store)
        P = 1.0 / (1.0 + np.exp(-F))
        return P.mean(axis=1), P.var(axis=1, ddof=1)


# ---- the laws the samplers are tested against ---------------------------------------------------------------------------------
def pg_moments(b, c):
    if c == 0:
        return b / 4.0, b / 24.0
    return b * math.tanh(c / 2) / (2 * c), b * (math.sinh(c) - c) / (4 * c ** 3 * math.cosh(c / 2) ** 2)


def pg1_series(n, c, rng, terms=200):
    """PG(1, c) by its defining Gamma series (1 / 2 pi^2) sum_k g_k / ((k - 1/2)^2 + c^2 / 4 pi^2), g_k ~ Exp(1), the first `terms`
    terms plus the mean of the dropped tail: an independent construction (NumPy's own generator)"""
    k = np.arange(1, terms + 1)
    den = (k - 0.5) ** 2 + c * c / (4 * math.pi ** 2)
    g = rng.standard_exponential((n, terms))
    kk = np.arange(terms + 1, 200001)
    tail = np.sum(1.0 / ((kk - 0.5) ** 2 + c * c / (4 * math.pi ** 2))) + 1.0 / 200000.5
    return (g @ (1.0 / den) + tail) / (2 * math.pi ** 2)


def ks_two_sample(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, allv, side="right") / len(a) - np.searchsorted(b, allv, side="right") / len(b))))


def ks_critical(alpha, n1, n2=None):
    c = math.sqrt(-math.log(alpha / 2) / 2)
    return c * math.sqrt((n1 + n2) / (n1 * n2)) if n2 else c / math.sqrt(n1)


# ---- the parity inputs (tests/test_gpu_mcgp.py compares chains; tests/test_mcgp_host.py asserts their margin condition) ---------
# name -> (likelihood, N, kernel kind, scale (number or D numbers), mean (None / number / "empirical"), seed of the chain,
#          n_samples, discard_initial, thinning): 20 sweeps each
CASES = {
    "logistic-173": ("logistic", 173, "sqexponential", 2.0, None, 11, 20, 0, 1),
    "logistic-200": ("logistic", 200, "sqexponential", 2.0, None, 12, 20, 0, 1),
    "studentt-173": ("studentt", 173, "sqexponential", 2.0, None, 13, 20, 0, 1),
    "studentt-200": ("studentt", 200, "sqexponential", 2.0, None, 14, 20, 0, 1),
    "negbinomial-173": ("negbinomial", 173, "sqexponential", 2.0, None, 15, 20, 0, 1),
    "negbinomial-200": ("negbinomial", 200, "sqexponential", 2.0, None, 16, 20, 0, 1),
    "logistic-constmean": ("logistic", 173, "sqexponential", 2.0, 0.3, 17, 20, 0, 1),
    "studentt-empmean": ("studentt", 200, "sqexponential", 2.0, "empirical", 18, 20, 0, 1),
    "logistic-ard-matern": ("logistic", 200, "matern52", (1.3, 2.2, 0.7), None, 19, 20, 0, 1),
    "logistic-thinned": ("logistic", 173, "sqexponential", 2.0, None, 20, 9, 3, 2),
}


def case_data(name, data_seed=3):
    """(X, y as the caller gives it, likelihood name, kernel kind, scale, mean values or None) of a parity case"""
    from _liks import labels

    likname, N, kind, scale, mean, seed, n, discard, thinning = CASES[name]
    rng = np.random.default_rng(data_seed)
    X = rng.random((N, 3))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7
    y = labels(likname, f, X, rng)
    if mean == "empirical":
        mean = 0.4 * np.cos(5 * X[:, 2])
    return X, y, likname, kind, scale, mean


def case_ref(name):
    """the restated model of a parity case and its sampling arguments (n, discard_initial, thinning)"""
    from _liks import oracle_lik

    X, y, likname, kind, scale, mean = case_data(name)
    _, N, _, _, _, seed, n, discard, thinning = CASES[name]
    lik = oracle_lik(R, likname)
    mu0 = None if mean is None else np.full(N, mean) if np.isscalar(mean) else mean
    rscale = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64)
    ref = MCGPRef(R.Kernel(kind, rscale, 1.5), lik, X, R.treat_labels(y, lik), seed, mu0=mu0)
    return ref, (n, discard, thinning)


def local_inputs(likname, n=300):
    """(y, f, seed, t) of the small agp_sample_local parity call: f on a grid with 0 and both signs, integer y for NegBinomial"""
    rng = np.random.default_rng(21)
    f = np.linspace(-6.0, 6.0, n)
    f[n // 2] = 0.0
    if likname == "logistic":
        y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    elif likname == "studentt":
        y = f + 0.5 * rng.standard_t(3, n)
    else:
        y = rng.integers(0, 12, n).astype(np.float64)
    return y, f, 77, 5
