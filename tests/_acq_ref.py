"""NumPy restatement of the acquisition functions and their multi-start ascent, written from the text of include/agp_hip.h
("ACQUISITION FUNCTIONS"), on top of tests/_predgrad_ref.py (the kernels' phi and phi', the squared distances).

    mu = k*' a,  var = v + jitter - k*' A k*  with W = K*m A' (W_ij = sum_l k*_il A[j][l]),  grad mu, grad var as predict_f_grad
    UCB = s mu + beta sigma;  EI = sigma (z Phi + phi);  PI = Phi;   z = (s (mu - best) - xi) / sigma
    grad alpha = d alpha / d mu  grad mu  +  d alpha / d sigma  grad var / (2 sigma)

Everything takes the six objects (Z, s, v, kind, a, A) of one latent, so a test can feed it the oracle's (the host suite: conditioning)
or the device's own `model.predictor()` (the GPU suite: parity).  dtype=np.float64 or np.longdouble; in the extended mode Phi comes
from mpmath (NumPy has no long-double erfc).  Also here: the trajectory cases both suites share.
"""
import functools
import math

import mpmath
import numpy as np
import scipy.special as sps

import _pathwise_max_ref as M
import _predgrad_cases as PC
import _predgrad_ref as G

PARITY = 1e-8  # the project's parity bound
COND_CAP = M.COND_CAP  # float64 against np.longdouble over a whole trajectory
GAP = M.GAP  # the index of the best start is compared where the two best values differ by more than GAP max|alpha|
JITTER = 1e-4  # the Float64 handles' jitter (the reference's constant)
KINDS = ("ucb", "ei", "pi")


def acq(kind, beta=0.0, best=0.0, xi=0.0, minimize=False):
    return dict(kind=kind, s=-1.0 if minimize else 1.0, beta=beta, best=best, xi=xi)


def _to_mp(t):
    hi = float(t)
    return mpmath.mpf(hi) + mpmath.mpf(float(t - np.longdouble(hi)))  # exact


def _ld(x):
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - mpmath.mpf(hi)))


with mpmath.workdps(40):
    PI_LD = _ld(mpmath.pi)


def Phi(z, dtype=np.float64):
    """erfc(-z / sqrt 2) / 2"""
    z = np.asarray(z, dtype=dtype)
    if np.dtype(dtype) == np.float64:
        return 0.5 * sps.erfc(-z * (1.0 / math.sqrt(2.0)))
    with mpmath.workdps(40):
        f = lambda t: _ld(mpmath.erfc(-_to_mp(t) / mpmath.sqrt(2)) / 2)
        return np.array([f(t) if np.isfinite(t) else t for t in z.ravel()], dtype=np.longdouble).reshape(z.shape)


def point(q, mu, var, dtype=np.float64):
    """(alpha, d alpha / d mu, d alpha / d sigma, d alpha / d var) of the moments; var <= 0 takes the limit, NaN moments give NaN"""
    T = np.dtype(dtype).type
    mu, var = np.asarray(mu, dtype=np.float64).astype(dtype), np.asarray(var, dtype=np.float64).astype(dtype)
    s, beta, best, xi = T(q["s"]), T(q["beta"]), T(q["best"]), T(q["xi"])
    pos = var > 0
    sg = np.sqrt(np.where(pos, var, T(1)))
    imp = s * (mu - best) - xi
    if q["kind"] == "ucb":
        al = np.where(pos, s * mu + beta * sg, s * mu)
        dm = np.full_like(mu, s)
        ds = np.where(pos, beta, T(0))
    else:
        z = imp / sg
        P, p = Phi(z, dtype), np.exp(-z * z / 2) / np.sqrt(2 * (T(np.pi) if np.dtype(dtype) == np.float64 else PI_LD))
        if q["kind"] == "ei":
            al = np.where(pos, sg * (z * P + p), np.maximum(imp, T(0)))
            dm = np.where(pos, s * P, np.where(imp > 0, s, T(0)))
            ds = np.where(pos, p, T(0))
        elif q["kind"] == "pi":
            al = np.where(pos, P, np.where(imp > 0, T(1), T(0)))
            dm = np.where(pos, s * p / sg, T(0))
            ds = np.where(pos, -z * p / sg, T(0))
        else:
            raise ValueError(q["kind"])
    dv = np.where(pos, ds / (2 * sg), T(0))
    bad = np.isnan(mu) | np.isnan(var)
    nan = T(np.nan)
    return tuple(np.where(bad, nan, t).astype(dtype) for t in (al, dm, ds, dv))


def moments(X, Z, s, v, kind, a, A, jitter=JITTER, dtype=np.float64):
    """(mu, var) in the arithmetic of dtype"""
    T = np.dtype(dtype).type
    X, Z, a, A = (np.asarray(x, dtype=np.float64).astype(dtype) for x in (X, Z, a, A))
    sc = np.broadcast_to(np.asarray(s, dtype=np.float64), (X.shape[1],)).astype(dtype)
    ks = T(v) * G.phi(kind, G.sqdist(X, Z, sc))
    W = ks @ A.T
    return ks @ a, (T(v) + T(jitter)) - np.sum(W * ks, axis=1)


def alpha_grad(q, X, parts, jitter=JITTER, dtype=np.float64):
    """(alpha (n,), grad (n, D), mu, var)"""
    Z, s, v, kind, a, A = parts
    mu, var = moments(X, Z, s, v, kind, a, A, jitter, dtype)
    gm, gv = G.grads(X, Z, s, v, kind, a, np.asarray(A).T, dtype=dtype)  # (W = K*m A': the device's index order)
    al, dm, _, dv = point(q, mu, var, dtype)
    return al, dm[:, None] * gm + dv[:, None] * gv, mu, var


def ascent(q, X0, parts, lo, hi, lr, steps, beta1=0.9, beta2=0.999, eps=1e-8, jitter=JITTER, dtype=np.float64):
    """(X (R, D), A (R,)): the final iterates and alpha there, by the recurrence of agp_pathwise_maximize on g = grad alpha"""
    T = np.dtype(dtype).type
    X0 = np.asarray(X0, dtype=np.float64).astype(dtype)
    D = X0.shape[1]
    lo, hi, lr = (np.broadcast_to(np.asarray(t, dtype=np.float64), (D,)).astype(dtype) for t in (lo, hi, lr))
    b1, b2, e = T(beta1), T(beta2), T(eps)
    x = np.minimum(np.maximum(X0, lo), hi)
    m, v = np.zeros_like(x), np.zeros_like(x)
    b1k, b2k = T(1), T(1)
    for _ in range(int(steps)):
        g = alpha_grad(q, x, parts, jitter, dtype)[1]
        m = b1 * m + (T(1) - b1) * g
        v = b2 * v + (T(1) - b2) * (g * g)
        b1k, b2k = b1k * b1, b2k * b2
        x = np.minimum(np.maximum(x + lr * ((m / (T(1) - b1k)) / (np.sqrt(v / (T(1) - b2k)) + e)), lo), hi)
    return x, alpha_grad(q, x, parts, jitter, dtype)[0]


def best(X, A):
    """(idx, x_best, a_best): the largest alpha, ties to the smallest index, a NaN never wins (all NaN: 0)"""
    idx, xb, ab = M.best(np.asarray(X)[None], np.asarray(A)[None])
    return int(idx[0]), xb[0], ab[0]


def top_gap(A):
    return float(M.top_gap(np.asarray(A, dtype=np.float64)[None])[0])


def relerr(a, b):
    """max |a - b| relative to max |b|"""
    return G.rel(a, b)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# One per axis value, not the product: m in {1, 63, 64, 65, 130}; D in {1, 3, 4, 5, 17, 33, 64} (the edges of the contraction's four
# dimension splits); starts R in {1, 63, 64, 65, 4096 + 37}; the three kernels with Scale and ARD transforms; SVGP Gaussian and
# Logistic, LogisticSoftMax latent 0 and 2, VGP, GP, a QuadratureVI SVGP, OnlineSVGP.  `pc` names the model and data of
# tests/_predgrad_cases.py; the D = 4, 5, 17, 33 cases are Gaussian SVGPs built here the same way.  T: the step counts of the
# trajectory tests (the 4133 starts run T = 1: they are there for the chunk boundary).
def _ard(D, base):
    return tuple(base * (0.8 + 0.1 * (d % 5)) * math.sqrt(3.0 / D) for d in range(D))


OWN = {  # the schema of _predgrad_cases.CASES
    "svgp-gaussian-d4-m65-m52-ard": dict(model="svgp", lik="gaussian", m=65, D=4, nt=255, kind="matern52", scale=_ard(4, 3.0), spread=1.0,
                                         mean=None),
    "svgp-gaussian-d5-m65-sq-ard": dict(model="svgp", lik="gaussian", m=65, D=5, nt=255, kind="sqexponential", scale=_ard(5, 3.0),
                                        spread=1.0, mean=None),
    "svgp-gaussian-d17-m65-m32-ard": dict(model="svgp", lik="gaussian", m=65, D=17, nt=255, kind="matern32", scale=_ard(17, 2.0),
                                          spread=1.0, mean=None),
    "svgp-gaussian-d33-m65-sq-ard": dict(model="svgp", lik="gaussian", m=65, D=33, nt=255, kind="sqexponential", scale=_ard(33, 2.0),
                                         spread=1.0, mean=None),
}
CASES = {
    "m130-d3-r4133": dict(pc="svgp-gaussian-m130-nt4133-sq-scale", R=4096 + 37, T=(1,)),
    "m65-logistic-m32-ard": dict(pc="svgp-logistic-m65-m32-ard", R=65, T=(1, 20)),
    "m1-r1": dict(pc="svgp-gaussian-m1-nt1-m52-scale", R=1, T=(1, 20)),
    "d1-m63-r63": dict(pc="svgp-logistic-d1-m63-m52-ard", R=63, T=(1, 20)),
    "d64-m64-r64": dict(pc="svgp-gaussian-d64-m64-sq-ard", R=64, T=(1, 20)),
    "softmax-latent0": dict(pc="svgp-softmax3-m65-sq-scale", R=65, T=(1, 20), latent=0),
    "softmax-latent2": dict(pc="svgp-softmax3-m65-sq-scale", R=65, T=(20,), latent=2),
    "vgp": dict(pc="vgp-n65-m32-scale", R=65, T=(1, 20)),
    "gp": dict(pc="gp-n65-sq-ard", R=65, T=(1, 20)),
    "quadrature": dict(pc="svgp-quadrature-m65", R=65, T=(20,)),
    "online": dict(pc="online-two-batches", R=65, T=(20,), spread=1.0, centre=(2.5, 1.0)),
    "d4": dict(pc="svgp-gaussian-d4-m65-m52-ard", R=65, T=(1, 20)),
    "d5": dict(pc="svgp-gaussian-d5-m65-sq-ard", R=65, T=(20,)),
    "d17": dict(pc="svgp-gaussian-d17-m65-m32-ard", R=65, T=(20,)),
    "d33": dict(pc="svgp-gaussian-d33-m65-sq-ard", R=65, T=(20,)),
}
TRAJECTORIES = [(n, k, t) for n, c in CASES.items() for k in KINDS for t in c["T"]]
XI = 0.01


def spec(name):
    """the _predgrad_cases-style description of a case's model"""
    pc = CASES[name]["pc"]
    return OWN[pc] if pc in OWN else PC.CASES[pc]


@functools.lru_cache(maxsize=None)
def own_data(pc):
    c = OWN[pc]
    rng = np.random.default_rng(211 + sum(map(ord, pc)))
    X = c["spread"] * rng.standard_normal((PC.NTRAIN, c["D"]))
    return dict(X=X, Xt=c["spread"] * rng.standard_normal((c["nt"], c["D"])), y=PC.labels(c["lik"], PC._f(X), X, rng),
                Z=X[rng.permutation(PC.NTRAIN)[:c["m"]]].copy(),
                idx=[np.sort(rng.choice(PC.NTRAIN, PC.B, replace=False)) for _ in range(PC.STEPS)])


def data(name):
    pc = CASES[name]["pc"]
    return own_data(pc) if pc in OWN else PC.data(pc)


@functools.lru_cache(maxsize=None)
def oracle_parts(name):
    """(Z, s, v, kind, a, A) of the case's latent on the oracle side (trained once, never mutated)"""
    pc, lat = CASES[name]["pc"], CASES[name].get("latent", 0)
    if pc not in OWN:
        return PC.reference(pc)["parts"][lat]
    c, d = OWN[pc], own_data(pc)
    ref = PC.R.SVGP(PC._rkernel(c), PC.oracle_lik(PC.R, c["lik"]), d["Z"], stochastic=True, batchsize=PC.B)
    ref.train(d["X"], d["y"], PC.STEPS, idx_stream=d["idx"])
    return PC._latent(ref.latents[0], ref.jitter)


def make_model(AGP, name):
    """the device side of a case, trained like the oracle side"""
    pc = CASES[name]["pc"]
    if pc not in OWN:
        return PC.make_model(AGP, pc)
    c, d = OWN[pc], own_data(pc)
    model = AGP.SVGP(PC._akernel(AGP, c), PC.agp_lik(AGP, c["lik"]), AGP.AnalyticSVI(PC.B), d["Z"], optimiser=False)
    AGP.train_(model, d["X"], d["y"], PC.STEPS, idx_stream=d["idx"])
    return model


def device_parts(model, name):
    """(Z, s, v, kind, a, A) with the DEVICE's own predictor objects: kernel and Z from the host mirror, (a, A) from model.predictor"""
    lat = CASES[name].get("latent", 0)
    cur = getattr(model, "_cur", None) or model  # OnlineSVGP: the model that owns the handle (padded inducing points included)
    a, A = model.predictor(lat)
    k = cur.kernels[lat]
    kind = {0: "sqexponential", 1: "matern52", 2: "matern32"}[k._kind]
    return np.asarray(cur.Zs[lat], dtype=np.float64), np.asarray(k.scales(cur.D), dtype=np.float64), float(k.variance), kind, a, A


def inputs(name):
    """(X0 (R, D), lo, hi, lr): the box [-2, 2] spread around the centre, starts uniform in +-1.3 spread -- 20 steps of about lr
    cannot reach a face from there -- except start 0, which lies outside the box in dimension 0 and is clipped; lr 0.03 spread"""
    c, sp_ = CASES[name], spec(name)
    D, R = sp_["D"], c["R"]
    spread = float(c.get("spread") or sp_["spread"])
    ctr = np.asarray(c.get("centre", np.zeros(D)), dtype=np.float64)
    rng = np.random.default_rng(3000 + 7 * R + D + sum(map(ord, name)))
    X0 = ctr + spread * rng.uniform(-1.3, 1.3, size=(R, D))
    X0[0, 0] = ctr[0] + 2.7 * spread
    return X0, ctr - 2.0 * spread, ctr + 2.0 * spread, np.full(D, 0.03 * spread)


def case_acq(kind, X0, parts, lo, hi):
    """the case's descriptor: UCB(2), or EI / PI with the largest posterior mean over the (clipped) starts as incumbent and xi = XI"""
    if kind == "ucb":
        return acq("ucb", beta=2.0)
    mu = moments(np.minimum(np.maximum(X0, lo), hi), *parts)[0]
    return acq(kind, best=float(np.max(mu)), xi=XI)
