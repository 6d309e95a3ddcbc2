"""The log predictive density lpd = log int p(y | f) N(f; mu, var) df restated from its definition (include/agp_hip.h, "LOG
PREDICTIVE DENSITY"), in two forms: float64 NumPy (lpd_np) and mpmath at 40 digits (lpd_mp) of the SAME sums -- Gaussian and
Laplace in closed form, the Gauss-Hermite sum over given nodes for Logistic, BayesianSVM, StudentT, Poisson, NegBinomial, the link
on the means for LogisticSoftMax / SoftMax -- and the integral itself by mpmath.quad (integral_mp), the yardstick of the closed
forms and of the rule's own error.  p(y | f) is the host mirror's likelihood_value (likelihoods.py:332-377) with labels +-1.

A likelihood is a tuple (name, p0, p1): ("gaussian", sigma2), ("laplace", beta), ("logistic",), ("bayesiansvm",),
("studentt", nu, sigma), ("poisson", lambda), ("negbinomial", r), ("logisticsoftmax", K), ("softmax", K)."""
import math

import mpmath as mp
import numpy as np
from scipy.special import erfc, erfcx, gammaln, logsumexp

QUAD = ("logistic", "bayesiansvm", "studentt", "poisson", "negbinomial")
MULTI = ("logisticsoftmax", "softmax")
DPS = 40


def gh_rule(n):
    """x_j = sqrt(2) t_j, w_j = omega_j / sqrt(pi): what the device receives (nvi.gauss_hermite_rule)"""
    t, om = np.polynomial.hermite.hermgauss(int(n))
    return np.ascontiguousarray(t * math.sqrt(2.0)), np.ascontiguousarray(om / math.sqrt(math.pi))


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def _log_sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, -np.log1p(np.exp(-np.abs(x))), x - np.log1p(np.exp(-np.abs(x))))


def _stirling_tail(z):
    i = 1.0 / z
    return i * (1.0 / 12.0 - i * i * (1.0 / 360.0 - i * i * (1.0 / 1260.0 - i * i / 1680.0)))


def lgamma_diff(y, r):
    """log Gamma(y + r) - log Gamma(y + 1) without cancelling two numbers of size y log y: from y = 32 on from Stirling's series
    lgamma(z) = (z - 1/2) log z - z + log(2 pi) / 2 + 1 / 12 z - 1 / 360 z^3 + 1 / 1260 z^5 - 1 / 1680 z^7 (next: z^-9 / 1188)"""
    y = np.asarray(y, dtype=np.float64)
    big = np.maximum(y, 32.0)
    st = ((big + 0.5) * np.log1p((r - 1.0) / (big + 1.0)) + (r - 1.0) * (np.log(big + r) - 1.0) + _stirling_tail(big + r)
          - _stirling_tail(big + 1.0))
    return np.where(y < 32.0, gammaln(y + r) - gammaln(y + 1.0), st)


def logp_np(lik, y, f):
    """log p(y | f), y and f broadcast"""
    name = lik[0]
    y = np.asarray(y, dtype=np.float64)
    if name == "logistic":
        return _log_sigmoid(y * f)
    if name == "bayesiansvm":
        z = y * f
        return _log_sigmoid(-2.0 * np.maximum(1.0 - z, 0.0) + 2.0 * np.maximum(1.0 + z, 0.0))
    if name == "studentt":
        nu, sig = lik[1], lik[2]
        c = math.lgamma(0.5 * (nu + 1.0)) - 0.5 * math.log(nu * math.pi) - math.lgamma(0.5 * nu)
        return c - 0.5 * (nu + 1.0) * np.log1p(((y - f) / sig) ** 2)
    if name == "poisson":
        lam = lik[1]
        ls = _log_sigmoid(f)
        return y * math.log(lam) - gammaln(y + 1.0) + np.where(y > 0, y * ls, 0.0) - lam * np.exp(ls)
    if name == "negbinomial":
        r = lik[1]
        return lgamma_diff(y, r) - math.lgamma(r) + r * _log_sigmoid(-f) + np.where(y > 0, y * _log_sigmoid(f), 0.0)
    raise ValueError(name)


def _laplace_logT(d, v, be):
    s = np.sqrt(v)
    a = (v / be - d) / (s * math.sqrt(2.0))
    with np.errstate(all="ignore"):
        lo = v / (2.0 * be * be) - d / be + np.log(erfc(np.minimum(a, 0.0)))
        hi = -0.5 * d * d / v + np.log(erfcx(np.maximum(a, 0.0)))
    return np.where(a < 0, lo, hi)


def lpd_np(lik, y, mu, var, x=None, w=None):
    """lpd[n] in float64.  Multi-class: y = 0-based class indices, mu (K, n)."""
    name = lik[0]
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if name == "gaussian":
        v = var + lik[1]
        return -0.5 * (np.log(2.0 * math.pi * v) + (np.asarray(y) - mu) ** 2 / v)
    if name == "laplace":
        d = np.asarray(y, dtype=np.float64) - mu
        return -math.log(4.0 * lik[1]) + np.logaddexp(_laplace_logT(d, var, lik[1]), _laplace_logT(-d, var, lik[1]))
    if name in MULTI:
        l = _log_sigmoid(mu) if name == "logisticsoftmax" else mu
        return l[np.asarray(y, dtype=np.int64), np.arange(mu.shape[1])] - logsumexp(l, axis=0)
    f = mu[:, None] + np.sqrt(var)[:, None] * np.asarray(x)[None, :]
    with np.errstate(divide="ignore"):
        lw = np.log(np.asarray(w))[None, :]
    return logsumexp(lw + logp_np(lik, np.asarray(y, dtype=np.float64)[:, None], f), axis=1)


# ---- mpmath, 40 digits -----------------------------------------------------------------------------------------------------------
def _mp_log_sigmoid(x):
    return -mp.log1p(mp.exp(-x)) if x >= 0 else x - mp.log1p(mp.exp(x))


def logp_mp(lik, y, f):
    name = lik[0]
    y = mp.mpf(float(y))
    if name == "logistic":
        return _mp_log_sigmoid(y * f)
    if name == "bayesiansvm":
        z = y * f
        return _mp_log_sigmoid(-2 * max(1 - z, mp.mpf(0)) + 2 * max(1 + z, mp.mpf(0)))
    if name == "studentt":
        nu, sig = mp.mpf(lik[1]), mp.mpf(lik[2])
        c = mp.loggamma((nu + 1) / 2) - mp.log(nu * mp.pi) / 2 - mp.loggamma(nu / 2)
        return c - (nu + 1) / 2 * mp.log1p(((y - f) / sig) ** 2)
    if name == "poisson":
        lam = mp.mpf(lik[1])
        ls = _mp_log_sigmoid(f)
        return y * mp.log(lam) - mp.loggamma(y + 1) + y * ls - lam * mp.exp(ls)
    if name == "negbinomial":
        r = mp.mpf(lik[1])
        return mp.loggamma(y + r) - mp.loggamma(y + 1) - mp.loggamma(r) + r * _mp_log_sigmoid(-f) + y * _mp_log_sigmoid(f)
    if name == "gaussian":
        return -(mp.log(2 * mp.pi * mp.mpf(lik[1])) + (y - f) ** 2 / mp.mpf(lik[1])) / 2
    if name == "laplace":
        return -abs(y - f) / mp.mpf(lik[1]) - mp.log(2 * mp.mpf(lik[1]))
    raise ValueError(name)


def _mp_logsumexp(ls):
    M = max(ls)
    return M + mp.log(mp.fsum(mp.exp(l - M) for l in ls))


def lpd_mp_point(lik, y, mu, var, x=None, w=None):
    """one point, the same sums as lpd_np at 40 digits (mu: the K means for a multi-class likelihood); an mpf"""
    name = lik[0]
    if name in MULTI:
        l = [_mp_log_sigmoid(mp.mpf(float(m))) if name == "logisticsoftmax" else mp.mpf(float(m)) for m in mu]
        return l[int(y)] - _mp_logsumexp(l)
    y, mu, var = mp.mpf(float(y)), mp.mpf(float(mu)), mp.mpf(float(var))
    if name == "gaussian":
        v = var + mp.mpf(lik[1])
        return -(mp.log(2 * mp.pi * v) + (y - mu) ** 2 / v) / 2
    if name == "laplace":
        be, d, s = mp.mpf(lik[1]), y - mu, mp.sqrt(var)
        T = lambda dd: mp.exp(var / (2 * be * be) - dd / be) * mp.erfc((var / be - dd) / (s * mp.sqrt(2)))  # noqa: E731
        return mp.log((T(d) + T(-d)) / (4 * be))
    s = mp.sqrt(var)
    return _mp_logsumexp([mp.log(mp.mpf(float(wj))) + logp_mp(lik, y, mu + s * mp.mpf(float(xj))) for xj, wj in zip(x, w) if wj > 0])


def lpd_mp(lik, y, mu, var, x=None, w=None):
    """lpd[n] as float64 of the 40-digit values"""
    with mp.workdps(DPS):
        if lik[0] in MULTI:
            mu = np.asarray(mu)
            return np.array([float(lpd_mp_point(lik, y[i], mu[:, i], None)) for i in range(mu.shape[1])])
        return np.array([float(lpd_mp_point(lik, yi, mi, vi, x, w)) for yi, mi, vi in zip(y, mu, var)])


def integral_mp(lik, y, mu, var, dps=30, degree=None):
    """log int p(y | f) N(f; mu, var) df by mpmath.quad, the interval split at y, y +- {1, 10, 100} width and mu +- {1, 4, 12} s
    (width: Laplace beta, StudentT sigma, else 1); an mpf at the caller's precision"""
    with mp.workdps(dps):
        y_, m, v = mp.mpf(float(y)), mp.mpf(float(mu)), mp.mpf(float(var))
        s = mp.sqrt(v)
        wd = mp.mpf(lik[1] if lik[0] == "laplace" else lik[2] if lik[0] == "studentt" else 1.0)
        centre = y_ if lik[0] in ("gaussian", "laplace", "studentt") else mp.mpf(0)
        pts = {centre, m}
        for k in (1, 10, 100):
            pts |= {centre - k * wd, centre + k * wd}
        for k in (1, 4, 12):
            pts |= {m - k * s, m + k * s}
        lo, hi = m - 40 * s, m + 40 * s  # (the Gaussian factor is below 1e-340 outside)
        pts = sorted(p for p in pts if lo < p < hi)
        # the integrand relative to its value at a reference point, so that nothing underflows at 1e-300
        ref = max(logp_mp(lik, y, p) - (p - m) ** 2 / (2 * v) for p in pts)
        g = lambda f: mp.exp(logp_mp(lik, y, f) - (f - m) ** 2 / (2 * v) - ref)  # noqa: E731
        kw = {} if degree is None else {"maxdegree": degree}
        val = mp.quad(g, [lo] + pts + [hi], **kw)
        return mp.log(val) + ref - mp.log(2 * mp.pi * v) / 2


def stable_integral(lik, y, mu, var, tol=1e-14):
    """(value as float, stable?): the integral at (dps 30, default degree) and at (dps 60, maxdegree 10), kept only if the two agree
    within tol * max(1, |value|): the integrator is then the yardstick, not the code under test"""
    a = integral_mp(lik, y, mu, var, 30)
    b = integral_mp(lik, y, mu, var, 60, degree=10)
    with mp.workdps(60):
        ok = abs(a - b) < tol * max(1, abs(b))
    return float(b), bool(ok)


# ---- the point-by-point grid (tests/test_lpd_host.py (a), tests/test_gpu_lpd.py (c)) -----------------------------------------------
GRID_LIKS = {
    "gaussian": ("gaussian", 0.05),
    "laplace": ("laplace", 0.4),
    "logistic": ("logistic",),
    "bayesiansvm": ("bayesiansvm",),
    "studentt": ("studentt", 3.0, 1.0),
    "poisson": ("poisson", 4.0),
    "negbinomial": ("negbinomial", 6.0),
    "logisticsoftmax": ("logisticsoftmax", 3),
    "softmax": ("softmax", 3),
}
GRID_NODES = (1, 3, 20, 100, 257)  # 257 is off the 16-lane grid
GRID_P = 1000
GOLDEN = "lpd/lpd_mp.npz"  # under tests/golden: the 40-digit values of the grid (tools/make_lpd_golden.py)


def grid(name):
    """(y, mu, var) of a likelihood: 1000 points, var from 1e-12 to 1e2, |mu| <= 30 (the grid of the quadrature kernel's test), plus
    the rows mu = -+800 y at var = 1e-2 for Logistic, |d| = 50 at var = 1e-3 and 30 for Laplace, and counts from 31 to 1e6 for
    NegBinomial"""
    rng = np.random.default_rng(sorted(GRID_LIKS).index(name) + 100)
    P = GRID_P
    if name in MULTI:
        K = GRID_LIKS[name][1]
        mu = rng.uniform(-30, 30, (K, P))
        var = 10.0 ** rng.uniform(-12, 2, (K, P))
        return rng.integers(0, K, P).astype(np.int32), mu, var
    mu = rng.uniform(-30, 30, P)
    var = 10.0 ** rng.uniform(-12, 2, P)
    var[:2] = (1e-12, 1e2)
    if name in ("logistic", "bayesiansvm"):
        y = np.sign(rng.standard_normal(P))
    elif name in ("poisson", "negbinomial"):
        y = rng.poisson(3.0, P).astype(np.float64)
    else:
        y = mu + 2.0 * rng.standard_normal(P)
    if name == "logistic":
        y[2:6] = (1.0, -1.0, 1.0, -1.0)
        mu[2:6] = (-800.0, 800.0, 800.0, -800.0)  # the first two: about -800, where a direct sum gives -inf
        var[2:6] = 1e-2
    if name == "negbinomial":  # counts at and beyond the switch of lgamma_diff
        y[2:8] = (31.0, 32.0, 33.0, 1000.0, 20000.0, 1e6)
    if name == "laplace":
        var[2:6] = (1e-3, 1e-3, 30.0, 30.0)
        y[2:6] = mu[2:6] + np.array([50.0, -50.0, 50.0, -50.0])
    return y, mu, var
