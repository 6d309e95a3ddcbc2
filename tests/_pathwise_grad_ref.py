"""NumPy restatement of the input gradients of pathwise samples, written from the specification in include/agp_hip.h
(agp_pathwise_eval_grad).  With t_ird = s_d (x_id - Z_rd), q_ir = sum_d t_ird^2 and c_ir = sigma2 phi'(q_ir),

    d f_s / d x_d (x_i) = - s_d sum_j amp sin(omega_j' (s o x_i) + p_j) omega_jd W_js  +  2 s_d sum_r c_ir t_ird V_rs

amp = sqrt(2 sigma2 / l), by direct differences of the scaled coordinates; phi' = d phi / d q in the closed forms that are finite at
r = 0.  `dtype` selects the arithmetic: np.longdouble gives the extended-precision evaluation of the same formula.
"""
import numpy as np

from _pathwise_ref import scales_of


def dphi(kind, q):
    """phi'(q), q = r^2 the squared scaled distance, for the three differentiable kernels"""
    T = q.dtype.type
    if kind == "sqexponential":
        return T(-0.5) * np.exp(T(-0.5) * q)
    r = np.sqrt(q)
    if kind == "matern52":
        s5 = np.sqrt(T(5))
        return -(T(5) / T(6)) * (T(1) + s5 * r) * np.exp(-s5 * r)
    if kind == "matern32":
        return T(-1.5) * np.exp(-np.sqrt(T(3)) * r)
    raise NotImplementedError("ExponentialKernel is not differentiable at zero distance")


def grad_tables(kind, scale, sigma2, Z, omega, phase, W, V, X, dtype=np.float64):
    """[S, n_t, D] from tables handed in: omega [l, D], phase [l], W [l, S], V [m, S]"""
    T = np.dtype(dtype).type
    X, Z = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype)
    omega, phase, W, V = (np.asarray(a, dtype=dtype) for a in (omega, phase, W, V))
    n, D = X.shape
    s = scales_of(scale, D).astype(dtype)
    amp = np.sqrt(T(2) * T(sigma2) / T(len(phase)))
    Xs, Zs = X * s, Z * s
    arg = np.zeros((n, len(phase)), dtype=dtype)
    q = np.zeros((n, len(Z)), dtype=dtype)
    for d in range(D):
        arg += Xs[:, d][:, None] * omega[:, d][None, :]
        t = Xs[:, d][:, None] - Zs[:, d][None, :]
        q += t * t
    A = -amp * np.sin(arg + phase[None, :])
    Cm = T(sigma2) * dphi(kind, q)
    G = np.empty((W.shape[1], n, D), dtype=dtype)
    for d in range(D):
        t = Xs[:, d][:, None] - Zs[:, d][None, :]
        G[:, :, d] = ((A * (s[d] * omega[:, d])[None, :]) @ W + (T(2) * s[d] * Cm * t) @ V).T
    return G


def grad(draw, X, dtype=np.float64):
    """[S, n_t, D] of a _pathwise_ref.Draw with V formed"""
    return grad_tables(draw.kind, draw.scale, draw.sigma2, draw.Z, draw.omega, draw.phase, draw.W, draw.V, X, dtype)
