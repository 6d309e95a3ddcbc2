"""NumPy restatement of the acquisition kinds that are evaluated in logarithms (LogEI, LogPI), written from the text of
csrc/agp_acq_log.h and of include/agp_hip.h ("ACQUISITION FUNCTIONS"), on top of tests/_acq_ref.py (the moments, the best-start rule,
the cases) and tests/_predgrad_ref.py (the gradients of the moments):

    z = (s (mu - best) - xi) / sigma,  h = phi + z Phi
    LogEI = log sigma + log h(z)   d/dmu = s Phi / (sigma h)     d/dsigma = phi / (sigma h)
    LogPI = log Phi(z)             d/dmu = s phi / (sigma Phi)   d/dsigma = -z phi / (sigma Phi)
    z >  -3: these expressions, Phi from erfc, log Phi = log1p(-Phi(-z)) for z > 0
    z <= -3: t = -z, c = 1 / (t + 2 / (t + 3 / (t + ...))) cut after the partial numerator 60 (t < 5), 32 (t < 12) or 12,
             R = 1 / (t + c), h / phi = c R

dtype=np.float64 or np.longdouble; in the extended mode Phi of the direct branch comes from mpmath (as in _acq_ref) and the continued
fraction runs in long double.  mpmath is the judge of both (tests/test_acq_log_host.py).
"""
import numpy as np

import _acq_batch_ref as B
import _acq_ref as A
import _pathwise_max_ref as M
import _predgrad_ref as G

KINDS = ("logei", "logpi")
CODES = {"logei": 5, "logpi": 6}  # AGP_ACQ_LOG_EI, AGP_ACQ_LOG_PI
PLAIN = {"logei": "ei", "logpi": "pi"}
BRANCH = -3.0
CF_TERMS = ((5.0, 60), (12.0, 32), (np.inf, 12))  # (t below, the last partial numerator)


def acq(kind, best=0.0, xi=0.0, minimize=False):
    return dict(kind=kind, s=-1.0 if minimize else 1.0, beta=0.0, best=best, xi=xi)


def continued_fraction(t, terms=None):
    """c = 1 / (t + 2 / (t + 3 / (t + ... terms / t))) from its tail, in t's dtype; terms=None: by the range of t, as the header"""
    T = t.dtype.type
    if terms is None:
        c = continued_fraction(t, CF_TERMS[-1][1])
        for below, n in CF_TERMS[-2::-1]:
            c = np.where(t < T(below), continued_fraction(t, n), c)
        return c
    u = np.zeros_like(t)
    for k in range(terms, 1, -1):
        u = T(k) / (t + u)
    return T(1) / (t + u)


def _direct(ei, s, z, sg, dtype):
    T = np.dtype(dtype).type
    two_pi = 2 * (T(np.pi) if np.dtype(dtype) == np.float64 else A.PI_LD)
    phi = np.exp(-z * z / 2) / np.sqrt(two_pi)
    if ei:
        P = A.Phi(z, dtype)
        h = phi + z * P
        return np.log(sg) + np.log(h), s * P / (sg * h), phi / (sg * h)
    up = z > 0
    Q = A.Phi(-np.abs(z), dtype)  # the smaller of Phi(z) and Phi(-z)
    P = np.where(up, T(1) - Q, Q)
    return np.where(up, np.log1p(-Q), np.log(Q)), s * phi / (sg * P), -z * phi / (sg * P)


def _tail(ei, s, z, sg, dtype):
    T = np.dtype(dtype).type
    two_pi = 2 * (T(np.pi) if np.dtype(dtype) == np.float64 else A.PI_LD)
    t = -z
    c = continued_fraction(t)
    tc = t + c  # 1 / R
    logphi = (T(-0.5) * z) * z - T(0.5) * np.log(two_pi)
    if ei:
        return logphi + (np.log(c) - np.log(tc) + np.log(sg)), s / (sg * c), tc / (sg * c)
    return logphi - np.log(tc), s * tc / sg, t * tc / sg


def point(q, mu, var, dtype=np.float64, branch=BRANCH):
    """(alpha, d alpha / d mu, d alpha / d sigma, d alpha / d var) of the moments; var <= 0 takes the limit, NaN moments give NaN.
    branch=+inf / -inf forces the continued fraction / the direct expressions (the tests compare the two at the branch point)"""
    T = np.dtype(dtype).type
    mu, var = (np.atleast_1d(np.asarray(t, dtype=np.float64)).astype(dtype) for t in (mu, var))
    s, best, xi = T(q["s"]), T(q["best"]), T(q["xi"])
    ei = q["kind"] == "logei"
    assert ei or q["kind"] == "logpi", q["kind"]
    al, dm, ds = (np.zeros(mu.shape, dtype=dtype) for _ in range(3))
    with np.errstate(all="ignore"):
        imp = s * (mu - best) - xi
        pos = var > 0
        sg = np.sqrt(np.where(pos, var, T(1)))
        z = imp / sg
        gain = ~pos & (imp > 0)
        al[~pos] = -np.inf
        al[gain] = np.log(imp[gain]) if ei else T(0)
        if ei:
            dm[gain] = s / imp[gain]
        direct = pos & (z > T(branch))
        for sel, f in ((direct, _direct), (pos & ~direct, _tail)):
            if np.any(sel):
                al[sel], dm[sel], ds[sel] = f(ei, s, z[sel], sg[sel], dtype)
        dv = np.where(pos, ds / (2 * sg), T(0))
    bad = np.isnan(mu) | np.isnan(var)
    return tuple(np.where(bad, T(np.nan), t).astype(dtype) for t in (al, dm, ds, dv))


def alpha_grad(q, X, parts, jitter=A.JITTER, dtype=np.float64, pending=None, tau2=0.0):
    """(log alpha (n,), its gradient (n, D), mu, var); with pending points the moments are those of _acq_batch_ref (the direct form)"""
    if pending is not None and len(pending):
        mu, var, gm, gv = B.moments_grads(X, parts, pending, tau2, jitter, dtype)
    else:
        Z, s, v, kind, a, Ap = parts
        mu, var = A.moments(X, Z, s, v, kind, a, Ap, jitter, dtype)
        gm, gv = G.grads(X, Z, s, v, kind, a, np.asarray(Ap).T, dtype=dtype)
    al, dm, _, dv = point(q, mu, var, dtype)
    return al, dm[:, None] * gm + dv[:, None] * gv, mu, var


def ascent(q, X0, parts, lo, hi, lr, steps, beta1=0.9, beta2=0.999, eps=1e-8, jitter=A.JITTER, dtype=np.float64):
    """_acq_ref.ascent, word for word, on the log kinds: (X (R, D), log alpha (R,)) of the final iterates"""
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


# ---- the judge and the grid -------------------------------------------------------------------------------------------------------------
ZS = (8.0, 1.0, 0.0, -0.5, -1.0, float(np.nextafter(-3.0, 0.0)), -3.0, float(np.nextafter(-3.0, -4.0)), -5.0, -12.0, -37.0, -38.0, -40.0,
      -100.0, -1e3, -1e6, -1e9)
SIGMAS = (1e-8, 1.0, 1e4)


def grid_moments(s=1.0):
    """(mu, var) with best = xi = 0: z = s mu / sqrt(var) up to the rounding of the product and the root, which the judge does not
    share -- it starts from these float64 numbers"""
    mu = np.array([s * z * sg for sg in SIGMAS for z in ZS])
    var = np.array([sg * sg for sg in SIGMAS for _ in ZS])
    return mu, var


def mp_point(kind, s, best, xi, mu, var, dps=100):
    """(log alpha, d / d mu, d / d sigma) from the defining expressions at `dps` digits, as floats; var > 0.  h = phi + z Phi cancels to
    1 / z^2 of its terms: 18 digits at z = -1e9, of 100"""
    import mpmath

    with mpmath.workdps(dps):
        mu, var, s, best, xi = (mpmath.mpf(float(t)) for t in (mu, var, s, best, xi))
        sg = mpmath.sqrt(var)
        z = (s * (mu - best) - xi) / sg
        P = mpmath.erfc(-z / mpmath.sqrt(2)) / 2
        p = mpmath.exp(-z * z / 2) / mpmath.sqrt(2 * mpmath.pi)
        if kind == "logei":
            h = p + z * P
            return float(mpmath.log(sg) + mpmath.log(h)), float(s * P / (sg * h)), float(p / (sg * h))
        return float(mpmath.log(P)), float(s * p / (sg * P)), float(-z * p / (sg * P))


def mp_grid(kind, s):
    mu, var = grid_moments(s)
    return np.array([mp_point(kind, s, 0.0, 0.0, m, v) for m, v in zip(mu, var)]).T


def err_alpha(got, want):
    """|got - want| / max(1, |want|), the measure of log alpha"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def err_rel(got, want):
    """|got - want| / |want| element by element, the measure of the derivatives (0 where both are 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))


# ---- the plateau case (tests/test_acq_log_host.py on the oracle's objects, tests/test_gpu_acq_log.py on the device's) -------------------
# The 1-D exact GP of _pathwise_max_ref.ONE_D (N = 40; with the noise variance 0.1, which keeps var = k** + jitter - k*' A k* well
# conditioned) and the incumbent 40 prior standard deviations above the largest posterior mean at the clipped starts: z <= -40
# everywhere in the box, where EI and PI and their gradients are exactly 0.  8 starts, 30 steps.
PLATEAU = dict(R=8, T=30, lr=0.01, sds=40.0, lo=-2.0, hi=0.6, noise=0.1)
PLATEAU_KINDS = (("ei", "logei"), ("pi", "logpi"))


def plateau_inputs():
    """(X0 (8, 1), lo, hi, lr): start 0 lies outside the box and is clipped onto its upper face, where log alpha rises inwards (towards
    the largest mean, at 0): it moves like the others"""
    X0 = np.concatenate([[2.6], np.linspace(-1.73, 0.45, PLATEAU["R"] - 1)])[:, None]
    return X0, np.array([PLATEAU["lo"]]), np.array([PLATEAU["hi"]]), np.array([PLATEAU["lr"]])


def plateau_oracle_parts():
    """(Z, s, v, kind, a, A) of the exact GP on the oracle's side"""
    from _gp_ref import GPRef
    from oracle import agp_ref as R

    c = M.ONE_D
    X, y = M.one_d_data()[:2]
    ref = GPRef(R.Kernel(c["kind"], c["scale"], c["sigma2"]), X, y, noise=PLATEAU["noise"], opt_noise=False)
    return ref.X, ref.kernel.scale, ref.kernel.sigma2, ref.kernel.kind, ref.alpha, (ref.Sinv + ref.Sinv.T) / 2


def plateau_model(AGP):
    c = M.ONE_D
    X, y = M.one_d_data()[:2]
    k = c["sigma2"] * (AGP.Matern52Kernel() @ AGP.ScaleTransform(c["scale"]))
    return AGP.GP(X, y, k, noise=PLATEAU["noise"], opt_noise=False, optimiser=False)


def plateau_best(parts, X0, lo, hi, jitter=A.JITTER):
    """max mu over the clipped starts + 40 sqrt(v + jitter)"""
    mu = A.moments(np.minimum(np.maximum(X0, lo), hi), *parts)[0]
    return float(np.max(mu)) + PLATEAU["sds"] * float(np.sqrt(parts[2] + jitter))


def device_parts(model, lat=0):
    """_acq_ref.device_parts for a model that is not one of its cases: kernel and Z from the host mirror, (a, A) from model.predictor"""
    a, Ap = model.predictor(lat)
    k = model.kernels[lat]
    kind = {0: "sqexponential", 1: "matern52", 2: "matern32"}[k._kind]
    return np.asarray(model.Zs[lat], dtype=np.float64), np.asarray(k.scales(model.D), dtype=np.float64), float(k.variance), kind, a, Ap
