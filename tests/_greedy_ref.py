"""NumPy restatement of the greedy conditional-variance selection (csrc/agp_greedy.h, `agp_greedy_variance`), and the cases the
host and GPU tests share (tests/test_greedy_host.py, tests/test_gpu_greedy.py).

    d_i = k(x_i, x_i) = variance ; for j = 0 .. m-1:
      p_j = argmax_i d_i (ties -> smaller index) ; stop if d_{p_j} <= tol * variance
      l_j = (k(X, x_{p_j}) - sum_{k<j} l_k l_k[p_j]) / sqrt(d_{p_j}) ; d <- d - l_j^2 ; d_{p_j} <- 0

Kernel values come from oracle.agp_ref.Kernel.  Besides the result the restatement records, per step, the pivot d_{p_j} and the
relative gap (d_{p_j} - second largest d) / d_{p_j}: the MARGIN by which the argmax was decided.  A parity case is one whose gaps
(after the first step, an exact tie by construction) and pivots are many orders above the rounding differences between device and
host arithmetic, so that no argmax can flip; tests/test_greedy_host.py asserts that of every case below.
"""
import numpy as np

from oracle.agp_ref import Kernel

MIN_GAP = 1e-6    # smallest relative top-two gap a parity case may have (steps 1 ..)
MIN_PIVOT = 1e-6  # smallest pivot, in units of the kernel variance

# name -> kernel (kind, scale or ARD scales, variance), sizes, data seed.  N off the 64 and 256 grids, m across a 64 boundary,
# D = 1, 2, 3, 33.  Long lengthscales on purpose: with short ones every untouched residual sits at ~variance and the gaps fall to
# 1e-9 .. 1e-15 (SqExponential at scale 6 in D = 3, Exponential at scale 3 in D = 33): such inputs cannot pin an argmax.
CASES = {
    "sqexp_d3": dict(kind="sqexponential", scale=2.0, variance=1.5, N=300, D=3, m=130, seed=3),
    "matern52_ard_d3": dict(kind="matern52", scale=(1.3, 2.2, 0.7), variance=1.5, N=300, D=3, m=130, seed=3),
    "matern32_d1": dict(kind="matern32", scale=1.4, variance=0.9, N=257, D=1, m=65, seed=3),
    "sqexp_d33": dict(kind="sqexponential", scale=0.5, variance=1.0, N=200, D=33, m=70, seed=3),
    "exponential_d2": dict(kind="exponential", scale=1.2, variance=1.1, N=300, D=2, m=130, seed=3),
}
KIND_ID = {"sqexponential": 0, "matern52": 1, "matern32": 2, "exponential": 3}


def case_kernel(case):
    c = CASES[case] if isinstance(case, str) else case
    sc = c["scale"]
    return Kernel(c["kind"], np.asarray(sc, dtype=np.float64) if np.ndim(sc) else float(sc), c["variance"])


def case_data(case):
    c = CASES[case] if isinstance(case, str) else case
    return np.random.default_rng(c["seed"]).random((c["N"], c["D"]))


def tiled_data(distinct=40, copies=5, D=3, seed=11):
    """`distinct` points repeated `copies` times: K_NN has rank `distinct`, the selection must stop there."""
    return np.tile(np.random.default_rng(seed).random((distinct, D)), (copies, 1))


def e2e_data():
    """The end-to-end classification problem: the first parity case's recipe and kernel at N = 500 (its first 300 rows are that
    case's X), labels from a smooth function."""
    c = CASES["sqexp_d3"]
    rng = np.random.default_rng(c["seed"])
    X = rng.random((500, c["D"]))
    y = np.sign(np.sin(4 * X[:, 0]) + X[:, 1] - 0.8 + 0.3 * rng.standard_normal(500))
    return X, y


def greedy(kernel, X, m, tol=1e-9):
    """-> dict(indices[m] (-1 behind `selected`), factor[N][m], resid[N], trace[m], pivots[m], gaps[m], selected)"""
    X = np.asarray(X, dtype=np.float64)
    N, var = X.shape[0], float(kernel.sigma2)
    d = np.full(N, var)
    F = np.zeros((N, m))
    idx = np.full(m, -1, dtype=np.int64)
    trace, pivots, gaps = np.zeros(m), np.zeros(m), np.full(m, np.nan)
    sel = 0
    for j in range(m):
        p = int(np.argmax(d))  # the first maximum: ties go to the smaller index
        if d[p] <= tol * var:
            break
        if N > 1:
            second = np.max(np.delete(d, p))
            gaps[j] = (d[p] - second) / d[p]
        pivots[j] = d[p]
        c = kernel.matrix(X, X[p:p + 1])[:, 0]
        l = (c - F[:, :j] @ F[p, :j]) / np.sqrt(d[p])
        F[:, j] = l
        d = d - l * l
        d[p] = 0.0  # a chosen point has no residual left and is never chosen again
        idx[j] = p
        trace[j] = np.sum(d)
        sel = j + 1
    return dict(indices=idx, factor=F, resid=d, trace=trace, pivots=pivots, gaps=gaps, selected=sel)


def subset_trace(kernel, X, idx):
    """tr(K_NN - K_NZ K_ZZ^-1 K_ZN) for Z = X[idx], with a plain Cholesky solve: independent of the restatement above."""
    X = np.asarray(X, dtype=np.float64)
    Z = X[np.asarray(idx)]
    Lz = np.linalg.cholesky(kernel.matrix(Z))
    A = np.linalg.solve(Lz, kernel.matrix(Z, X))  # Lz^-1 K_ZN
    return float(np.sum(kernel.diag(X)) - np.sum(A * A))


def margins(res):
    """(smallest relative top-two gap over the steps after the first, smallest pivot) of a restatement result"""
    k = res["selected"]
    return float(np.min(res["gaps"][1:k])), float(np.min(res["pivots"][:k]))


_cache = {}


def case_result(case):
    """The restatement of a named case, computed once and shared; callers must not modify it."""
    if case not in _cache:
        c = CASES[case]
        X = case_data(case)
        res = greedy(case_kernel(case), X, c["m"])
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        X.setflags(write=False)
        _cache[case] = (X, res)
    return _cache[case]
