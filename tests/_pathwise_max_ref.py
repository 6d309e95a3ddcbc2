"""NumPy restatement of the multi-start ascent of pathwise samples, written from the specification in include/agp_hip.h
(agp_pathwise_maximize), on top of tests/_pathwise_ref.py and tests/_pathwise_grad_ref.py (grad_tables).  A particle (s, r) starts at
x0[s, r] clipped into [lo, hi] and takes T ADAM steps k = 1 .. T on path s,

    g = sign grad f_s(x) ;  m = beta1 m + (1 - beta1) g ;  v = beta2 v + (1 - beta2) g o g
    x = min(max(x + lr o (m / (1 - b1)) / (sqrt(v / (1 - b2)) + eps), lo), hi)

with b1 = beta1^k, b2 = beta2^k as running products; F is f_s at the final x.  `dtype` selects the arithmetic (np.longdouble: the
extended-precision evaluation of the same iteration).  The tables are handed in, so a test can evaluate it on the device's own.

Also here: the cases that the host and the GPU tests of the ascent share (CASES, case_inputs) and a host surrogate for their tables
(surrogate_tables), so that the conditioning of every case is checked without a device.
"""
import math

import numpy as np

import _pathwise_grad_ref as PG
import _pathwise_ref as P


def phi_base(kind, q):
    """phi(q), q = r^2 the squared scaled distance"""
    T = q.dtype.type
    if kind == "sqexponential":
        return np.exp(T(-0.5) * q)
    r = np.sqrt(q)
    if kind == "matern52":
        s5 = np.sqrt(T(5))
        return (T(1) + s5 * r + T(5) * q / T(3)) * np.exp(-s5 * r)
    if kind == "matern32":
        s3 = np.sqrt(T(3))
        return (T(1) + s3 * r) * np.exp(-s3 * r)
    raise NotImplementedError("ExponentialKernel is not differentiable at zero distance")


def value_tables(kind, scale, sigma2, Z, omega, phase, W, V, X, dtype=np.float64):
    """the paths [S, n_t] from tables handed in, in the arithmetic of dtype: sum_j amp cos(a_j) W_js + sum_r sigma2 phi(q_r) V_rs"""
    T = np.dtype(dtype).type
    X, Z = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype)
    omega, phase, W, V = (np.asarray(a, dtype=dtype) for a in (omega, phase, W, V))
    n, D = X.shape
    s = P.scales_of(scale, D).astype(dtype)
    amp = np.sqrt(T(2) * T(sigma2) / T(len(phase)))
    Xs, Zs = X * s, Z * s
    arg = np.zeros((n, len(phase)), dtype=dtype)
    q = np.zeros((n, len(Z)), dtype=dtype)
    for d in range(D):
        arg += Xs[:, d][:, None] * omega[:, d][None, :]
        t = Xs[:, d][:, None] - Zs[:, d][None, :]
        q += t * t
    return ((amp * np.cos(arg + phase[None, :])) @ W + (T(sigma2) * phi_base(kind, q)) @ V).T


def _own(fn, tb, X, dtype, *model):
    """fn(..., X[s]) of path s alone, for every s: [S, R] or [S, R, D]"""
    kind, scale, sigma2, Z = model
    return np.stack([fn(kind, scale, sigma2, Z, tb["omega"], tb["phase"], tb["W"][:, s:s + 1], tb["V"][:, s:s + 1], X[s], dtype)[0]
                     for s in range(X.shape[0])])


def values(kind, scale, sigma2, Z, tb, X, dtype=np.float64):
    """F[s, r] = f_s(X[s, r])"""
    return _own(value_tables, tb, X, dtype, kind, scale, sigma2, Z)


def grads(kind, scale, sigma2, Z, tb, X, dtype=np.float64):
    """G[s, r, :] = grad f_s (X[s, r])"""
    return _own(PG.grad_tables, tb, X, dtype, kind, scale, sigma2, Z)


def ascent(kind, scale, sigma2, Z, tb, X0, lo, hi, lr, steps, beta1=0.9, beta2=0.999, eps=1e-8, minimize=False, dtype=np.float64):
    """(X [S, R, D], F [S, R]): the final iterates and their values.  X0 is [S, R, D], or [R, D] for starts shared by the S paths."""
    T = np.dtype(dtype).type
    S = np.asarray(tb["W"]).shape[1]
    X0 = np.asarray(X0, dtype=dtype)
    if X0.ndim == 2:
        X0 = np.broadcast_to(X0, (S,) + X0.shape)
    D = X0.shape[2]
    lo, hi, lr = (np.broadcast_to(np.asarray(a, dtype=dtype), (D,)) for a in (lo, hi, lr))
    b1, b2, e, sign = T(beta1), T(beta2), T(eps), T(-1 if minimize else 1)
    x = np.minimum(np.maximum(X0, lo), hi)
    m, v = np.zeros_like(x), np.zeros_like(x)
    b1k, b2k = T(1), T(1)
    for _ in range(int(steps)):
        g = sign * grads(kind, scale, sigma2, Z, tb, x, dtype)
        m = b1 * m + (T(1) - b1) * g
        v = b2 * v + (T(1) - b2) * (g * g)
        b1k, b2k = b1k * b1, b2k * b2
        x = np.minimum(np.maximum(x + lr * ((m / (T(1) - b1k)) / (np.sqrt(v / (T(1) - b2k)) + e)), lo), hi)
    return x, values(kind, scale, sigma2, Z, tb, x, dtype)


def best(X, F, minimize=False):
    """(idx [S], x_best [S, D], f_best [S]): per path the largest sign f, ties to the smallest start, a NaN never wins (all NaN: 0)"""
    key = np.where(np.isnan(F), -np.inf, -F if minimize else F).astype(np.float64)
    idx = np.argmax(key, axis=1)  # the first of equal maxima; a row of -inf gives 0
    rows = np.arange(len(idx))
    return idx, X[rows, idx], F[rows, idx]


def top_gap(F, minimize=False):
    """per path the difference of the two best values, relative to max|F| (inf for a single start)"""
    F = np.asarray(F, dtype=np.float64)
    if F.shape[1] < 2:
        return np.full(F.shape[0], np.inf)
    srt = np.sort(-F if minimize else F, axis=1)
    return (srt[:, -1] - srt[:, -2]) / np.max(np.abs(F))


# ---- the cases shared by tests/test_pathwise_maximize_host.py and tests/test_gpu_pathwise_maximize.py ------------------------------
SIGMA2 = 1.5
STEPS = (1, 20)
COND_CAP = 1e-11  # float64 against np.longdouble over the whole trajectory
GAP = 1e-6  # best_idx is compared where the two best values of a path differ by more than GAP max|f|


def ard(D):
    """ARD scales around sqrt(3 / D), as tests/test_gpu_pathwise_grad.py: squared scaled distances of a few units in every D"""
    return tuple((0.8 + 0.1 * (d % 5)) * math.sqrt(3.0 / D) for d in range(D))


# model: svgp (m inducing points), vgp / gp (N = m = 130 training points), lsm (LogisticSoftMax, 3 latents)
CASES = {
    "m63-l1-S1-R65-D3-sqexp": dict(model="svgp", m=63, nf=1, S=1, R=65, D=3, kind="sqexponential", scale=3.0, shared=False),
    "m64-l65-S5-R13-D3-m52-ard": dict(model="svgp", m=64, nf=65, S=5, R=13, D=3, kind="matern52", scale=ard(3), shared=True),
    "m65-l200-S65-R1-D1-m32": dict(model="svgp", m=65, nf=200, S=65, R=1, D=1, kind="matern32", scale=ard(1), shared=False),
    "m130-l65-S5-R65-D33-sqexp-ard": dict(model="svgp", m=130, nf=65, S=5, R=65, D=33, kind="sqexponential", scale=ard(33), shared=False),
    "m65-l65-S5-R13-D64-m52-ard": dict(model="svgp", m=65, nf=65, S=5, R=13, D=64, kind="matern52", scale=ard(64), shared=True),
    "m64-l65-S65-R65-D3-sqexp": dict(model="svgp", m=64, nf=65, S=65, R=65, D=3, kind="sqexponential", scale=3.0, shared=False),
    "vgp-N130-m52": dict(model="vgp", m=130, nf=65, S=5, R=13, D=3, kind="matern52", scale=3.0, shared=False),
    "gp-N130-m32": dict(model="gp", m=130, nf=200, S=5, R=13, D=3, kind="matern32", scale=3.0, shared=False),
    "lsm-latent0": dict(model="lsm", m=65, nf=65, S=5, R=13, D=3, kind="sqexponential", scale=3.0, shared=False, latent=0),
    "lsm-latent2": dict(model="lsm", m=65, nf=65, S=5, R=13, D=3, kind="sqexponential", scale=3.0, shared=True, latent=2),
}
SEED, T_DRAW = 77, 3  # of every case's draw


def case_inputs(name):
    """(X0, lo, hi, lr) of a case: the box [-2, 2]^D, starts uniform in [-1.3, 1.3]^D -- 20 steps of at most ~lr cannot reach a face
    from there, so no two particles of a path end on the same corner with the same value -- except start 0, which lies outside the
    box in dimension 0 and is clipped; step sizes 0.03 .. 0.036 by dimension."""
    c = CASES[name]
    S, R, D = c["S"], c["R"], c["D"]
    rng = np.random.default_rng(1000 + 7 * S + 3 * R + D)
    X0 = rng.uniform(-1.3, 1.3, size=(R, D) if c["shared"] else (S, R, D))
    X0[..., 0, 0] = 2.7
    lo, hi = np.full(D, -2.0), np.full(D, 2.0)
    lr = 0.03 * (1.0 + 0.1 * (np.arange(D) % 3))
    return X0, lo, hi, lr


def case_Z(name):
    """the inducing points of a case's host surrogate: standard normal, m x D"""
    c = CASES[name]
    return np.random.default_rng(500 + c["m"] + c["D"]).standard_normal((c["m"], c["D"]))


def surrogate_tables(name):
    """A case without a device: Omega, the phases and W are the device's bit for bit (the stream contract); V comes from a posterior
    of the same kind as the trained one -- mu = the tests' target function on Z, -2 eta2 = K^-1 + 4 I -- through Matheron's rule.
    The GPU tests repeat the conditioning check on the device's own tables."""
    c = CASES[name]
    Z = case_Z(name)
    d = P.Draw(c["kind"], c["scale"], SIGMA2, Z, c["S"], c["nf"], SEED, T_DRAW, latent=c.get("latent", 0))
    K = P.kernel(c["kind"], c["scale"], SIGMA2, Z, Z) + 1e-4 * np.eye(len(Z))
    mu = np.sin(2 * Z[:, 0]) + 0.5 * Z[:, min(1, c["D"] - 1)] ** 2 - 0.7
    d.sparse(mu, -0.5 * (np.linalg.inv(K) + 4.0 * np.eye(len(Z))))
    return Z, dict(omega=d.omega, phase=d.phase, W=d.W, V=d.V)


# ---- the 1-D maximum: an exact GP on 40 points of 2 exp(-x^2) cos 3x, 64 uniform starts, against a grid of 200 ----------------------
ONE_D = dict(kind="matern52", scale=2.0, sigma2=1.5, noise=0.01, N=40, S=8, nf=200, seed=11, t=0, R=64, T=100, lr=0.005, lo=-2.0, hi=2.0)


def one_d_data():
    """(X, y, X0 [64, 1], grid [200, 1])"""
    c = ONE_D
    X = np.linspace(-1.9, 1.9, c["N"])[:, None]
    y = 2.0 * np.exp(-X[:, 0] ** 2) * np.cos(3 * X[:, 0]) + 0.05 * np.random.default_rng(5).standard_normal(c["N"])
    return X, y, np.linspace(c["lo"], c["hi"], c["R"])[:, None], np.linspace(c["lo"], c["hi"], 200)[:, None]
