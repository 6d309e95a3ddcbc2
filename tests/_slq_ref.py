"""Plain NumPy Float64 restatement of the stochastic-Lanczos-quadrature log-determinant of `IterativeGP.log_marginal_likelihood`
(csrc/agp_kmv_host.h: cg_solve_slq, cg_probes): pivoted partial Cholesky preconditioner P = L L' + sigma2 I, one preconditioned CG per
probe, the CG coefficients -> the Lanczos tridiagonal T -> eigh -> e1' log(T) e1, and
    log det M ~= log det P + (1/t) sum_c (z_c' P^-1 z_c) e1' log(T_c) e1 .
With the exact-trace probes (base samples sqrt(t) I, t = n + k: sum_c z_c z_c' = t P) the estimate equals log det M once every CG has
converged, so its deviation from the eigvalsh value measures the recurrence's own rounding: the GPU test takes 16 times the worst
deviation at its shapes as its bound.  NumPy only.
"""
import numpy as np


def pivoted_cholesky(K, rank, stop=1e-12):
    """the n x k factor of the greedy (largest residual diagonal first) partial Cholesky of K, k <= rank"""
    n = len(K)
    d, L = np.diag(K).copy(), np.zeros((n, 0))
    for _ in range(min(rank, n)):
        p = int(np.argmax(d))
        if d[p] <= stop * K[p, p]:
            break
        col = (K[:, p] - L @ L[p]) / np.sqrt(d[p])
        L, d = np.column_stack([L, col]), d - col * col
    return L


def pcg_coefficients(M, Pinv, b, tol, max_iter):
    """(alphas, betas, b' P^-1 b) of preconditioned CG on M x = b, stopped at |r| <= tol |b|"""
    x, r = np.zeros_like(b), b.copy()
    z = Pinv @ r
    p, rz, al, be = z.copy(), r @ z, [], []
    bpb = rz
    for _ in range(max_iter):
        q = M @ p
        a = rz / (p @ q)
        x, r = x + a * p, r - a * q
        al.append(a)
        if np.sqrt(r @ r) <= tol * np.sqrt(b @ b):
            break
        z = Pinv @ r
        rz_new = r @ z
        be.append(rz_new / rz)
        p, rz = z + be[-1] * p, rz_new
    return np.array(al), np.array(be[:len(al) - 1]), bpb


def e1_log_e1(al, be):
    m = len(al)
    T = np.diag(1.0 / al)
    for j in range(1, m):
        T[j, j] += be[j - 1] / al[j - 1]
        T[j, j - 1] = T[j - 1, j] = np.sqrt(be[j - 1]) / al[j - 1]
    lam, Q = np.linalg.eigh(T)
    return float(np.sum(Q[0] ** 2 * np.log(lam)))


def exact_trace_logdet(K, sigma2, rank, tol=1e-12, max_iter=1000):
    """(the estimate with exact-trace probes, log det by eigvalsh, L)"""
    n = len(K)
    M = K + sigma2 * np.eye(n)
    L = pivoted_cholesky(K, rank)
    k = L.shape[1]
    P = L @ L.T + sigma2 * np.eye(n)
    Pinv = np.linalg.inv(P)
    t = n + k
    probes = np.sqrt(t) * np.column_stack([np.sqrt(sigma2) * np.eye(n), L])
    acc = 0.0
    for c in range(t):
        al, be, bpb = pcg_coefficients(M, Pinv, probes[:, c], tol, max_iter)
        acc += bpb * e1_log_e1(al, be)
    logdetP = (n - k) * np.log(sigma2) + np.linalg.slogdet(sigma2 * np.eye(k) + L.T @ L)[1]
    return logdetP + acc / t, float(np.sum(np.log(np.linalg.eigvalsh(M)))), L
