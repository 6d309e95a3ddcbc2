"""NumPy restatement of the joint Monte-Carlo batch acquisition (include/agp_hip.h, "ACQUISITION FUNCTIONS", paragraph "Joint
batches"), written from the forward definition:

    mu_j = k*(x_j)' a,   C = k(X, X) - K* A K*' + jitter I  (its lower triangle is what a Cholesky reads),   C = L L',   f_s = mu + L eps_s
    q-EI  = mean_s max(0, max_j (s (f_sj - best) - xi)),     q-UCB = mean_s max_j (s mu_j + beta sqrt(pi/2) |(L eps_s)_j|)

The gradient is NOT the device's algebra (a reverse pass through the factor): it is the TANGENT of the forward definition.  For the
direction "member j, coordinate d" the tangents d mu and d C follow from d k / d x, the tangent of the factor is
d L = L Phi(L^-1 dC L^-T) with Phi = strict lower triangle plus half the diagonal, and alpha is linear in (d mu, d L) once every
sample's winner is fixed.  tests/test_acq_joint_host.py checks it against central differences of this file's own alpha.

Everything takes the six objects (Z, s, v, kind, a, A) of one latent (tests/_acq_ref.py) and works in dtype = np.float64 or
np.longdouble, batched over the sets.  Also here: the inputs and cases that the host and the GPU suite share.
"""
import functools

import numpy as np

import _acq_ref as A
import _mcvi_ref as MC
import _predgrad_ref as G

JITTER = A.JITTER
KINK = 1e-7  # a sample's winner is separated from the runner-up and from zero by more than KINK max|f_sj - best| of the set
STREAM = 3  # the stream of the mirror's default base samples: agp_mc_normals(ctx, seed, t=0, stream=3, S, q + n)
MAX_Q, MAX_S = 16, 4096


def base_samples(S, K, seed=0):
    """the table the mirror draws without base_samples=, bit for bit (tests/_mcvi_ref.py)"""
    return MC.normals(int(seed), 0, STREAM, int(S), int(K))


def _cast(parts, dtype):
    Z, s, v, kind, a, Ap = parts
    Z, a, Ap = (np.asarray(t, dtype=np.float64).astype(dtype) for t in (Z, a, Ap))
    sc = np.broadcast_to(np.asarray(s, dtype=np.float64), (Z.shape[1],)).astype(dtype)
    return Z, sc, np.dtype(dtype).type(v), kind, a, Ap


def members(X, P, dtype=np.float64):
    """(n, q', D): the q optimised members of every set, then the pending ones"""
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    if P is None or len(P) == 0:
        return X
    P = np.asarray(P, dtype=np.float64).astype(dtype)
    return np.concatenate([X, np.broadcast_to(P[None], (X.shape[0],) + P.shape)], axis=1)


def from_lower(M):
    """the symmetric matrix whose lower triangle is M's"""
    return np.tril(M) + np.swapaxes(np.tril(M, -1), -1, -2)


def _pairs(Xa, sc):
    """t_jld = s_d (x_jd - x_ld) and q_jl = sum_d t^2, ascending d"""
    t = sc * (Xa[:, :, None, :] - Xa[:, None, :, :])
    q = np.zeros(t.shape[:3], dtype=Xa.dtype)
    for d in range(Xa.shape[-1]):
        q += t[..., d] * t[..., d]
    return t, q


def moments(X, parts, P=None, jitter=JITTER, dtype=np.float64):
    """(mu (n, q'), C (n, q', q'), K (n, q', m)) of the sets X (n, q, D) with the pending points P"""
    Z, sc, v, kind, a, Ap = _cast(parts, dtype)
    Xa = members(X, P, dtype)
    n, qp, D = Xa.shape
    K = (v * G.phi(kind, G.sqdist(Xa.reshape(n * qp, D), Z, sc))).reshape(n, qp, -1)
    _, qq = _pairs(Xa, sc)
    C = v * G.phi(kind, qq) - K @ Ap @ np.swapaxes(K, 1, 2) + np.dtype(dtype).type(jitter) * np.eye(qp, dtype=dtype)
    return K @ a, from_lower(C), K


def chol(C):
    """the lower factor, batched over the leading axes (NumPy has no long-double LAPACK)"""
    L = np.zeros_like(C)
    for k in range(C.shape[-1]):
        d = np.sqrt(C[..., k, k] - np.sum(L[..., k, :k] * L[..., k, :k], axis=-1))
        L[..., k, k] = d
        if k + 1 < C.shape[-1]:
            L[..., k + 1:, k] = (C[..., k + 1:, k] - np.einsum("...jk,...k->...j", L[..., k + 1:, :k], L[..., k, :k])) / d[..., None]
    return L


def inv_lower(L):
    X = np.zeros_like(L)
    eye = np.eye(L.shape[-1], dtype=L.dtype)
    for i in range(L.shape[-1]):
        X[..., i, :] = (eye[i] - np.einsum("...k,...kc->...c", L[..., i, :i], X[..., :i, :])) / L[..., i, i, None]
    return X


def _root_half_pi(dtype):
    return np.sqrt((np.dtype(dtype).type(np.pi) if np.dtype(dtype) == np.float64 else A.PI_LD) / 2)


def samples(q, mu, L, eps, dtype=np.float64):
    """per sample: (value of the winner (n, S), winner (n, S), counts (n, S), d value / d (L eps)_winner (n, S), margin (n,)).
    margin: the smallest distance of a winner from its runner-up and from the kink at zero (the improvement for q-EI, (L eps)_j for
    q-UCB with beta > 0), relative to the largest |f_sj - best| of the set"""
    T = np.dtype(dtype).type
    s, beta, best, xi = T(q["s"]), T(q["beta"]), T(q["best"]), T(q["xi"])
    eps = np.asarray(eps, dtype=np.float64).astype(dtype)
    z = np.einsum("njk,sk->nsj", L, eps)
    f = mu[:, None, :] + z
    if q["kind"] == "ei":
        val = s * (f - best) - xi
    elif q["kind"] == "ucb":
        val = s * mu[:, None, :] + (beta * _root_half_pi(dtype)) * np.abs(z)
    else:
        raise ValueError(q["kind"])
    win = np.argmax(val, axis=-1)  # the first maximum
    top = np.take_along_axis(val, win[..., None], axis=-1)[..., 0]
    zw = np.take_along_axis(z, win[..., None], axis=-1)[..., 0]
    if val.shape[-1] > 1:
        gap = top - np.sort(val, axis=-1)[..., -2]
    else:
        gap = np.full_like(top, np.inf)
    if q["kind"] == "ei":
        counts, dz, zero = top > 0, np.full_like(top, s), np.abs(top)
        term = np.where(counts, top, T(0))
    else:
        counts, dz = np.ones(top.shape, dtype=bool), np.sign(zw) * (beta * _root_half_pi(dtype))
        zero = np.abs(zw) if q["beta"] > 0 else np.full_like(top, np.inf)
        term = top
    scale = np.max(np.abs(f - best), axis=(1, 2))
    margin = np.min(np.minimum(gap, zero), axis=1) / scale
    return term, win, counts, dz, margin


def alpha_grad(q, X, parts, eps, P=None, jitter=JITTER, dtype=np.float64, grad=True):
    """(alpha (n,), grad (n, q, D) or None, margin (n,)) of the sets X (n, q, D)"""
    T = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64)
    nq = X.shape[1]
    mu, C, K = moments(X, parts, P, jitter, dtype)
    L = chol(C)
    term, win, counts, dz, margin = samples(q, mu, L, eps, dtype)
    S = T(term.shape[1])
    alpha = np.sum(term, axis=1) / S
    if not grad:
        return alpha, None, margin
    Z, sc, v, kind, a, Ap = _cast(parts, dtype)
    Xa = members(X, P, dtype)
    n, qp, D = Xa.shape
    e = np.asarray(eps, dtype=np.float64).astype(dtype)
    # alpha is linear in (d mu, d L) with the winners fixed: alpha' = sum_j mbar_j dmu_j + sum_jk Gbar_jk dL_jk
    hot = (win[..., None] == np.arange(qp)) & counts[..., None]  # (n, S, q')
    mbar = T(q["s"]) * np.sum(hot, axis=1).astype(dtype) / S
    Gbar = np.einsum("nsa,sk->nak", hot.astype(dtype) * dz[..., None], e) / S
    # the tangents of k*(x_j), mu_j and C for the direction (j, d), j < q
    tz = Xa[:, :nq, None, :] - Z[None, None]  # (n, q, m, D)
    qz = np.zeros(tz.shape[:3], dtype=dtype)
    for d in range(D):
        qz += (sc[d] * tz[..., d]) ** 2
    dK = np.swapaxes(2 * (v * G.dphi(kind, qz))[..., None] * (sc * sc) * tz, 2, 3)  # (n, q, D, m)
    dmu = dK @ a
    u_row = np.einsum("njdm,nlm->njdl", dK, K @ Ap.T)  # dk_j' A k_l: the tangent of (K A K')_jl in x_j
    u_col = np.einsum("njdm,nlm->njdl", dK, K @ Ap)  # k_l' A dk_j: that of (K A K')_lj
    t, qq = _pairs(Xa, sc)
    dkxx = 2 * (v * G.dphi(kind, qq))[:, :nq, None, :] * sc[None, None, :, None] * np.swapaxes(t[:, :nq], 2, 3)  # (n, q, D, q')
    dC = np.zeros((n, nq, D, qp, qp), dtype=dtype)
    for j in range(nq):
        dC[:, j, :, j, :j] = dkxx[:, j, :, :j] - u_row[:, j, :, :j]
        dC[:, j, :, j + 1:, j] = dkxx[:, j, :, j + 1:] - u_col[:, j, :, j + 1:]
        dC[:, j, :, j, j] = -(u_row[:, j, :, j] + u_col[:, j, :, j])
    dC = from_lower(dC)
    Li = inv_lower(L)
    M = np.einsum("nab,njdbc,nec->njdae", Li, dC, Li)
    Phi = np.tril(M, -1) + np.einsum("...aa->...a", M)[..., None] * (np.eye(qp, dtype=dtype) / 2)
    dL = np.einsum("nab,njdbc->njdac", L, Phi)
    g = mbar[:, :nq, None] * dmu + np.einsum("nak,njdak->njd", Gbar, dL)
    return alpha, g, margin


def ascent(q, X0, parts, eps, lo, hi, lr, steps, P=None, beta1=0.9, beta2=0.999, eps_adam=1e-8, jitter=JITTER, dtype=np.float64):
    """(X (R, q, D), A (R,), margin): the final tuples, alpha there, and the smallest kink margin met along the trajectory, by the
    recurrence of agp_pathwise_maximize on every coordinate of every member"""
    T = np.dtype(dtype).type
    X0 = np.asarray(X0, dtype=np.float64).astype(dtype)
    D = X0.shape[-1]
    lo, hi, lr = (np.broadcast_to(np.asarray(t, dtype=np.float64), (D,)).astype(dtype) for t in (lo, hi, lr))
    b1, b2, e = T(beta1), T(beta2), T(eps_adam)
    x = np.minimum(np.maximum(X0, lo), hi)
    m, v = np.zeros_like(x), np.zeros_like(x)
    b1k, b2k = T(1), T(1)
    worst = np.inf
    for _ in range(int(steps)):
        _, g, mg = alpha_grad(q, x, parts, eps, P, jitter, dtype)
        worst = min(worst, float(np.min(mg)))
        m = b1 * m + (T(1) - b1) * g
        v = b2 * v + (T(1) - b2) * (g * g)
        b1k, b2k = b1k * b1, b2k * b2
        x = np.minimum(np.maximum(x + lr * ((m / (T(1) - b1k)) / (np.sqrt(v / (T(1) - b2k)) + e)), lo), hi)
    al, _, mg = alpha_grad(q, x, parts, eps, P, jitter, dtype, grad=False)
    return x, al, min(worst, float(np.min(mg)))


def best(X, Al):
    """(idx, X_best (q, D), a_best): a tuple is one row for the best-start rule"""
    X = np.asarray(X)
    idx, _, ab = A.best(X.reshape(len(X), -1), Al)
    return idx, X[idx], ab


# ---- the inputs both suites share -------------------------------------------------------------------------------------------------------
# One per axis value, not the product: q in {1, 2, 3, 16}; S in {1, 63, 64, 65, 257}; n_pending in {0, 1, 16 - q}; the model cases of
# the issue; 1366 sets of q = 3 cross the chunk of floor(4096 / 3) = 1365 sets with a ragged tuple.  (case, q, n_pending, S, sets, seed):
# the seed is the input's own -- a drawn input that met a kink got another one, the condition stayed.
VALUES = [
    ("m65-logistic-m32-ard", 3, 0, 64, 5, 0),
    ("m65-logistic-m32-ard", 1, 0, 1, 65, 0),
    ("m65-logistic-m32-ard", 2, 1, 63, 7, 0),
    ("m65-logistic-m32-ard", 16, 0, 65, 3, 0),
    ("m65-logistic-m32-ard", 3, 13, 257, 3, 0),
    ("m65-logistic-m32-ard", 1, 15, 64, 4, 0),
    ("m65-logistic-m32-ard", 2, 14, 65, 3, 0),
    ("m65-logistic-m32-ard", 3, 1, 64, 1366, 0),
    ("m1-r1", 2, 1, 63, 4, 0),
    ("d1-m63-r63", 3, 1, 64, 5, 0),
    ("d64-m64-r64", 3, 1, 65, 3, 0),
    ("d64-m64-r64", 16, 0, 64, 2, 0),
    ("gp", 3, 0, 257, 5, 0),
    ("vgp", 2, 1, 64, 5, 0),
    ("online", 3, 1, 63, 5, 0),
]
ASCENTS = [(name, T) for name in ("m65-logistic-m32-ard", "gp", "d5") for T in (1, 20)]  # q = 3, S = 64
ASCENT_Q, ASCENT_S, ASCENT_R = 3, 64, 9
DIRECTIONS = [("ei", False), ("ei", True), ("ucb", False), ("ucb", True)]


def value_id(c):
    return f"{c[0]}-q{c[1]}-n{c[2]}-S{c[3]}-sets{c[4]}"


def _box(name):
    c, sp_ = A.CASES[name], A.spec(name)
    D = sp_["D"]
    spread = float(c.get("spread") or sp_["spread"])
    ctr = np.asarray(c.get("centre", np.zeros(D)), dtype=np.float64)
    return D, spread, ctr


@functools.lru_cache(maxsize=None)
def sets(name, q, n, nsets, seed=0):
    """(X (sets, q, D), P (n, D)): tuples and pending points uniform in +-1.3 spread around the case's centre (the box of
    _acq_ref.inputs is +-2 spread)"""
    D, spread, ctr = _box(name)
    rng = np.random.default_rng(9000 + 131 * q + 17 * n + nsets + 1009 * seed + sum(map(ord, name)))
    X = ctr + spread * rng.uniform(-1.3, 1.3, size=(nsets, q, D))
    P = ctr + spread * rng.uniform(-1.3, 1.3, size=(n, D))
    return X, P


@functools.lru_cache(maxsize=None)
def table(S, K, seed=0):
    return base_samples(S, K, 77 + seed)


def case_acq(kind, minimize, X, P, parts):
    """UCB(2), or EI with xi = XI and the best posterior mean over the case's own points as incumbent: improvements of both signs"""
    if kind == "ucb":
        return A.acq("ucb", beta=2.0, minimize=minimize)
    pts = np.vstack([np.asarray(X).reshape(-1, np.shape(X)[-1]), P])
    mu = A.moments(pts, *parts)[0]
    return A.acq("ei", best=float(np.min(mu) if minimize else np.max(mu)), xi=A.XI, minimize=minimize)


def ascent_inputs(name, seed=0):
    """(X0 (R, 3, D), P (1, D), lo, hi, lr): starts as in _acq_ref.inputs -- the box [-2, 2] spread, starts within +-1.3 spread, member 0
    of start 0 outside the box in dimension 0 -- and one pending point"""
    D, spread, ctr = _box(name)
    rng = np.random.default_rng(4100 + D + 1009 * seed + sum(map(ord, name)))
    X0 = ctr + spread * rng.uniform(-1.3, 1.3, size=(ASCENT_R, ASCENT_Q, D))
    X0[0, 0, 0] = ctr[0] + 2.7 * spread
    P = ctr + spread * rng.uniform(-1.3, 1.3, size=(1, D))
    return X0, P, ctr - 2.0 * spread, ctr + 2.0 * spread, np.full(D, 0.03 * spread)


def degenerate(name):
    """(X (2, 3, D), P (1, D)): set 0 has two identical members, set 1 a member on an inducing point (the pending one is ordinary)"""
    X, P = sets(name, 3, 1, 2, 5)
    X = X.copy()
    X[0, 2] = X[0, 0]
    d = A.data(name)
    X[1, 1] = (d["Z"] if "Z" in d else d["X"])[0]
    return X, P


def one_member_inputs(name, kind, parts):
    """(X (n, 1, D), acq) for the q = 1 identities: UCB(2), or EI with the mean of the posterior means as incumbent and the drawn
    points with |z| <= 2 -- chosen by z alone: there EI is no rare event of the table's 4096 draws, so that the table estimates its
    own standard error"""
    X, _ = sets(name, 1, 0, 64, 1)
    if kind == "ucb":
        return X, A.acq("ucb", beta=2.0)
    mu, var = A.moments(X[:, 0], *parts)
    q = A.acq("ei", best=float(np.mean(mu)), xi=A.XI)
    z = (mu - q["best"] - q["xi"]) / np.sqrt(var)
    return X[np.abs(z) <= 2.0], q


def one_member_terms(q, mu, var, eps):
    """(n, S): the summands of alpha with one member, (imp + sigma eps_s)^+ or s mu + beta sqrt(pi/2) sigma |eps_s|"""
    sg = np.sqrt(var)
    e = np.asarray(eps)[:, 0]
    if q["kind"] == "ei":
        return np.maximum((q["s"] * (mu - q["best"]) - q["xi"])[:, None] + q["s"] * sg[:, None] * e[None], 0.0)
    return q["s"] * mu[:, None] + q["beta"] * np.sqrt(np.pi / 2) * sg[:, None] * np.abs(e)[None]
