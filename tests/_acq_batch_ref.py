"""NumPy restatement of batch acquisition with pending points, written from the text of include/agp_hip.h ("ACQUISITION FUNCTIONS",
paragraph "Pending points"), on top of tests/_acq_ref.py (the point function, the moments, the best-start rule) and
tests/_predgrad_ref.py (phi, phi', the squared distances, the gradients of the moments).  The DIRECT form:

    cov(x, x') = k(x, x') - k*(x)' A k*(x')                      (no jitter)
    C_ij = cov(p_i, p_j) + (jitter + tau2) [i == j],   c_j(x) = cov(x, p_j)
    mu_P = mu,   var_P = var - c' C^-1 c,   grad var_P = grad var - 2 (dc/dx)' C^-1 c
    alpha_P = A(mu, var_P), its gradient by the chain rule

in np.float64 or np.longdouble (C^-1 by a hand-written Cholesky: NumPy has no long-double solver; n <= 64).  The greedy batch is the
recurrence of _acq_ref.ascent on alpha_P, then _acq_ref.best, round after round.  The device computes the augmented-predictor form
by bordering; `augmented` and `border` restate those two for the host tests, which tie them to the direct form.

Also here: the pending sets and the cases that tests/test_acq_batch_host.py and tests/test_gpu_acq_batch.py share.
"""
import functools

import numpy as np

import _acq_ref as A
import _predgrad_ref as G

JITTER = A.JITTER
NOISES = (0.0, 0.01)


# ---- the direct form ------------------------------------------------------------------------------------------------------------------
def _cast(parts, dtype):
    Z, s, v, kind, a, Ap = parts
    Z, a, Ap = (np.asarray(t, dtype=np.float64).astype(dtype) for t in (Z, a, Ap))
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), (Z.shape[1],)).astype(dtype)
    return Z, s, np.dtype(dtype).type(v), kind, a, Ap


def cholesky(C):
    """lower L with L L' = C, in C's own dtype"""
    n = len(C)
    L = np.zeros_like(C)
    for j in range(n):
        d = C[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is {d}")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (C[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def chol_solve(L, B):
    """(L L')^-1 B, column by column, in L's dtype"""
    n = len(L)
    Y = np.array(B, dtype=L.dtype, copy=True)
    for i in range(n):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def cov(X, Y, parts, dtype=np.float64):
    """cov(x_i, y_j) of the latent's posterior, (len(X), len(Y)); no jitter"""
    Z, s, v, kind, _, Ap = _cast(parts, dtype)
    X, Y = (np.asarray(t, dtype=np.float64).astype(dtype) for t in (X, Y))
    kx, ky = v * G.phi(kind, G.sqdist(X, Z, s)), v * G.phi(kind, G.sqdist(Y, Z, s))
    return v * G.phi(kind, G.sqdist(X, Y, s)) - kx @ Ap @ ky.T


def pending_factor(P, tau2, parts, jitter=JITTER, dtype=np.float64):
    """the Cholesky factor of C"""
    T = np.dtype(dtype).type
    return cholesky(cov(P, P, parts, dtype) + (T(jitter) + T(tau2)) * np.eye(len(P), dtype=dtype))


def moments_grads(X, parts, P, tau2, jitter=JITTER, dtype=np.float64):
    """(mu, var_P, grad mu, grad var_P) at the rows of X"""
    Z, s, v, kind, a, Ap = _cast(parts, dtype)
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    mu, var = A.moments(X, *parts, jitter=jitter, dtype=dtype)
    gm, gv = G.grads(X, parts[0], parts[1], parts[2], kind, parts[4], np.asarray(parts[5]).T, dtype=dtype)
    P = np.asarray(P, dtype=np.float64).astype(dtype).reshape(-1, X.shape[1])
    if len(P) == 0:
        return mu, var, gm, gv
    L = pending_factor(P, tau2, parts, jitter, dtype)
    c = cov(X, P, parts, dtype)  # (n_t, n)
    S = chol_solve(L, c.T).T  # rows C^-1 c(x_i)
    var_p = var - np.sum(c * S, axis=1)
    # dc_j / dx_d = 2 s_d^2 [v phi'(q(x, p_j)) (x_d - p_jd) - sum_l v phi'(q(x, z_l)) (x_d - z_ld) (A k*(p_j))_l]
    cz, cp = v * G.dphi(kind, G.sqdist(X, Z, s)), v * G.dphi(kind, G.sqdist(X, P, s))
    AkP = Ap @ (v * G.phi(kind, G.sqdist(P, Z, s))).T  # (m, n)
    gvp = np.empty_like(gv)
    for d in range(X.shape[1]):
        dc = 2 * s[d] * s[d] * (cp * (X[:, d][:, None] - P[None, :, d]) - (cz * (X[:, d][:, None] - Z[None, :, d])) @ AkP)
        gvp[:, d] = gv[:, d] - 2 * np.sum(dc * S, axis=1)
    return mu, var_p, gm, gvp


def alpha_grad(q, X, parts, P, tau2, jitter=JITTER, dtype=np.float64):
    """(alpha_P (n,), grad alpha_P (n, D), mu, var_P)"""
    mu, var, gm, gv = moments_grads(X, parts, P, tau2, jitter, dtype)
    al, dm, _, dv = A.point(q, mu, var, dtype)
    return al, dm[:, None] * gm + dv[:, None] * gv, mu, var


def ascent(q, X0, parts, P, tau2, lo, hi, lr, steps, beta1=0.9, beta2=0.999, eps=1e-8, jitter=JITTER, dtype=np.float64):
    """_acq_ref.ascent, word for word, on alpha_P"""
    T = np.dtype(dtype).type
    X0 = np.asarray(X0, dtype=np.float64).astype(dtype)
    D = X0.shape[1]
    lo, hi, lr = (np.broadcast_to(np.asarray(t, dtype=np.float64), (D,)).astype(dtype) for t in (lo, hi, lr))
    b1, b2, e = T(beta1), T(beta2), T(eps)
    x = np.minimum(np.maximum(X0, lo), hi)
    m, v = np.zeros_like(x), np.zeros_like(x)
    b1k, b2k = T(1), T(1)
    for _ in range(int(steps)):
        g = alpha_grad(q, x, parts, P, tau2, jitter, dtype)[1]
        m = b1 * m + (T(1) - b1) * g
        v = b2 * v + (T(1) - b2) * (g * g)
        b1k, b2k = b1k * b1, b2k * b2
        x = np.minimum(np.maximum(x + lr * ((m / (T(1) - b1k)) / (np.sqrt(v / (T(1) - b2k)) + e)), lo), hi)
    return x, alpha_grad(q, x, parts, P, tau2, jitter, dtype)[0]


def batch(q, nq, X0, parts, P, tau2, lo, hi, lr, steps, jitter=JITTER, dtype=np.float64):
    """the greedy batch: a list over the rounds of dict(idx, x, a, X, A).  The winner joins the pending set as the float64 number
    that the interface hands on (x_b is an output of the call)"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, np.shape(X0)[1])
    rounds = []
    for _ in range(nq):
        X, Al = ascent(q, X0, parts, P, tau2, lo, hi, lr, steps, jitter=jitter, dtype=dtype)
        idx, xb, ab = A.best(X, Al)
        rounds.append(dict(idx=idx, x=xb, a=ab, X=X, A=Al))
        P = np.vstack([P, np.asarray(xb, dtype=np.float64)[None]])
    return rounds


# ---- the equivalent form and its bordering (what the device computes) -------------------------------------------------------------------
def augmented(parts, P, tau2, jitter=JITTER, dtype=np.float64):
    """(Z', a', A') by the block formula: A' = [[A + V C^-1 V', -V C^-1], [-C^-1 V', C^-1]], V = A K_ZP"""
    Z, s, v, kind, a, Ap = _cast(parts, dtype)
    P = np.asarray(P, dtype=np.float64).astype(dtype)
    n = len(P)
    Ci = chol_solve(pending_factor(P, tau2, parts, jitter, dtype), np.eye(n, dtype=dtype))
    V = Ap @ (v * G.phi(kind, G.sqdist(Z, P, s)))
    return np.vstack([Z, P]), np.concatenate([a, np.zeros(n, dtype=dtype)]), np.block([[Ap + V @ Ci @ V.T, -V @ Ci], [-Ci @ V.T, Ci]])


def border(parts, P, tau2, jitter=JITTER, dtype=np.float64):
    """(Z', a', A') by bordering in the order p_1, p_2, ...: k' = k(Z', p), w = A' k', c = (v + jitter + tau2) - k'' w,
    A'' = [[A' + w w'/c, -w/c], [-w'/c, 1/c]]; also the list of the pivots c"""
    T = np.dtype(dtype).type
    Z, s, v, kind, a, Ap = _cast(parts, dtype)
    cs = []
    for p in np.asarray(P, dtype=np.float64).astype(dtype):
        k = v * G.phi(kind, G.sqdist(Z, p[None], s))[:, 0]
        w = Ap @ k
        c = (v + T(jitter) + T(tau2)) - k @ w
        cs.append(c)
        Ap = np.block([[Ap + np.outer(w, w) / c, -w[:, None] / c], [-w[None] / c, np.full((1, 1), 1 / c, dtype=dtype)]])
        Z, a = np.vstack([Z, p[None]]), np.concatenate([a, np.zeros(1, dtype=dtype)])
    return Z, a, Ap, cs


def var_augmented(X, parts, Zp, Apr, jitter=JITTER, dtype=np.float64):
    """(v + jitter) - k'(x)' A' k'(x)"""
    T = np.dtype(dtype).type
    _, s, v, kind, _, _ = _cast(parts, dtype)
    k = v * G.phi(kind, G.sqdist(np.asarray(X, dtype=np.float64).astype(dtype), Zp, s))
    return (v + T(jitter)) - np.sum((k @ Apr) * k, axis=1)


# ---- the pending sets and the cases ---------------------------------------------------------------------------------------------------------
# The padding and tile edges of m' = m + n: m' = 64 (63 + 1), m' = 65 (64 + 1), n = 63 on m = 1, and n = 5 on the model classes; the
# chunk of 4096 test points is crossed by m130-d3-r4133.
PENDING = {"d1-m63-r63": 1, "d64-m64-r64": 1, "m1-r1": 63, "m65-logistic-m32-ard": 5, "gp": 5, "vgp": 5, "softmax-latent2": 5, "online": 5,
           "m130-d3-r4133": 5}


@functools.lru_cache(maxsize=None)
def _pending(name, n):
    X0, lo, hi, _ = A.inputs(name)
    c = A.spec(name)
    rng = np.random.default_rng(9000 + 31 * n + sum(map(ord, name)))
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    P = ctr + 0.65 * half * rng.uniform(-1.0, 1.0, size=(n, len(lo)))  # inside the starts' region of the box
    if c["kind"] != "sqexponential":  # a Matern kernel at zero distance: on an inducing point (a training input of the VGP)
        d = A.data(name)
        P[0] = d["Z"][0] if "Z" in d else d["X"][0]
    if n >= 2:
        P[n - 1] = P[n // 2]  # a duplicate
    P.setflags(write=False)
    return P


def pending(name, n=None):
    """the case's pending points (n, D): in the Matern cases the first lies on the first inducing point (the same float64 numbers on
    the oracle's side and the device's: Z is data), with n >= 2 the last is a duplicate of the one in the middle"""
    return _pending(name, PENDING[name] if n is None else n).copy()


def eval_points(name):
    """the case's Xt and the pending points themselves"""
    return np.vstack([A.data(name)["Xt"], pending(name)])


# (name, kind, tau2, n_pending, q, T): q = 4, T = 20 on the three model classes with UCB and EI at both noises; PI where its rounds keep
# a top gap (not on `gp`); d64-m64-r64 so that m' passes 64 during the rounds; the 4133 starts for the chunk; one batch with
# pending points handed in
BATCHES = ([(n, k, t, 0, 4, 20) for n in ("gp", "m65-logistic-m32-ard", "vgp") for k in ("ucb", "ei") for t in NOISES]
           + [(n, "pi", 0.0, 0, 4, 20) for n in ("m65-logistic-m32-ard", "vgp", "d64-m64-r64")]
           + [("d64-m64-r64", "ucb", 0.0, 0, 4, 20), ("m130-d3-r4133", "ucb", 0.0, 0, 2, 1), ("m65-logistic-m32-ard", "ucb", 0.01, 2, 3, 20)])


def batch_id(b):
    return "-".join(str(t) for t in b)


def conditioning(rounds64, roundsld, lo, hi):
    """(x difference over the box, alpha difference, smallest top gap, indices equal) over the rounds of a batch in both arithmetics"""
    box = float(np.max(np.asarray(hi) - np.asarray(lo)))
    ex = max(float(np.max(np.abs(r["X"] - l["X"]))) / box for r, l in zip(rounds64, roundsld))
    ea = max(A.relerr(r["A"], l["A"]) for r, l in zip(rounds64, roundsld))
    gap = min(A.top_gap(r["A"]) for r in rounds64)
    return ex, ea, gap, all(r["idx"] == l["idx"] for r, l in zip(rounds64, roundsld))
