"""NumPy restatement of the input gradients of the predictive moments (include/agp_hip.h, "PREDICTIVE GRADIENTS"), per latent:

    q_ij = sum_d s_d^2 (x_id - z_jd)^2,   c_ij = v phi'(q_ij)
    dmu_i  / dx_d =  2 s_d^2 sum_j a_j        c_ij (x_id - z_jd)
    dvar_i / dx_d = -4 s_d^2 sum_j (k*_i A)_j c_ij (x_id - z_jd)        k*_ij = v phi(q_ij)

with phi' in the forms that are finite at r = 0 (nothing divides by r).  It takes the six objects (Z, s, v, kind, a, A) of one latent
-- `latent_parts` reads them off an oracle model -- and has two modes: dtype=np.float64 and dtype=np.longdouble (every intermediate in
that type; inputs are the same float64 numbers).  The agreement of the two modes is the conditioning of a test case.
"""
import numpy as np
import scipy.linalg as sla

KINDS = ("sqexponential", "matern32", "matern52")


def phi(kind, q):
    if kind == "sqexponential":
        return np.exp(-q / 2)
    r = np.sqrt(q)
    if kind == "matern32":
        s3 = np.sqrt(q.dtype.type(3))
        return (1 + s3 * r) * np.exp(-s3 * r)
    if kind == "matern52":
        s5 = np.sqrt(q.dtype.type(5))
        return (1 + s5 * r + 5 * q / 3) * np.exp(-s5 * r)
    raise ValueError(kind)


def dphi(kind, q):
    """d phi / d q, q = r^2"""
    if kind == "sqexponential":
        return -np.exp(-q / 2) / 2
    r = np.sqrt(q)
    if kind == "matern32":
        s3 = np.sqrt(q.dtype.type(3))
        return -(q.dtype.type(3) / 2) * np.exp(-s3 * r)
    if kind == "matern52":
        s5 = np.sqrt(q.dtype.type(5))
        return -(q.dtype.type(5) / 6) * (1 + s5 * r) * np.exp(-s5 * r)
    raise ValueError(kind)


def sqdist(X, Z, s):
    q = np.zeros((len(X), len(Z)), dtype=X.dtype)
    for d in range(X.shape[1]):  # ascending d, direct differences
        t = s[d] * (X[:, d][:, None] - Z[None, :, d])
        q += t * t
    return q


def grads(X, Z, s, v, kind, a, A=None, dtype=np.float64):
    """(dmu, dvar), each (n, D); dvar is None without A"""
    T = np.dtype(dtype).type
    X, Z, a = (np.asarray(x, dtype=np.float64).astype(dtype) for x in (X, Z, a))
    D = X.shape[1]
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), (D,)).astype(dtype)
    v = T(v)
    q = sqdist(X, Z, s)
    c = v * dphi(kind, q)
    Pm = c * a[None, :]
    Pv = None
    if A is not None:
        W = (v * phi(kind, q)) @ np.asarray(A, dtype=np.float64).astype(dtype)
        Pv = c * W
    dmu = np.empty((len(X), D), dtype=dtype)
    dvar = None if A is None else np.empty((len(X), D), dtype=dtype)
    for d in range(D):
        diff = X[:, d][:, None] - Z[None, :, d]
        dmu[:, d] = 2 * s[d] * s[d] * np.sum(Pm * diff, axis=1)
        if A is not None:
            dvar[:, d] = -4 * s[d] * s[d] * np.sum(Pv * diff, axis=1)
    return dmu, dvar


def moments(X, Z, s, v, kind, a, A, jitter=0.0):
    """(mu, var) of the same restatement: what the gradients are the gradients of (float64)"""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), (X.shape[1],))
    ks = v * phi(kind, sqdist(X, Z, s))
    return ks @ a, v + jitter - np.einsum("ij,jk,ik->i", ks, A, ks)


def latent_parts(kernel, Z, L, mu, Sigma):
    """(Z, s, v, kind, a, A) of a variational latent of the oracle: a = K^-1 mu, A = K^-1 - K^-1 Sigma K^-1 with K = L L' -- the
    two objects the oracle's predict_f forms (oracle/agp_ref.py, SVGP.predict_f)"""
    m = len(Z)
    a = sla.cho_solve((L, True), mu)
    SK = sla.cho_solve((L, True), Sigma.T).T
    A = sla.cho_solve((L, True), np.eye(m) - SK)
    return (np.asarray(Z, dtype=np.float64), kernel.scale, kernel.sigma2, kernel.kind, a, (A + A.T) / 2)


def mix(A, gq, square=False):
    """multi-output: out_t = sum_q A[t][q]^p g_q"""
    A = np.asarray(A)
    W = A * A if square else A
    return [sum(W[t, q] * gq[q] for q in range(A.shape[1])) for t in range(A.shape[0])]


def rel(a, b):
    """relative error in max norm"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.longdouble(1e-300)))
