"""Extended-precision reference and element-wise error budget for the kernel-matrix kernels (csrc/agp_cavi.h: k_kernelmatrix_mma,
k_kernelmatrix).  NumPy only; shared by tests/test_kmat_budget_host.py (CPU) and tests/test_gpu_kernelmatrix_edges.py (GPU).

Reference
    The device scales a coordinate with ONE IEEE multiply in T, x[d] * T(scale_d) (the staging loops of both kernels and k_scale_rows);
    np.multiply in dtype T reproduces that bit for bit (`scaled`).  From those rounded values everything else is np.longdouble:
    direct differences, d2 = sum_d (sx_d - sy_d)^2, s2 = |sx|^2 + |sy|^2 and the kernel function.  The GEMM form
    |sx|^2 + |sy|^2 - 2 sx.sy is never used here.

Budget (derived, not measured).  u = unit roundoff of T, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, Lemma 3.1),
Dp = ceil(D / 8) * 8 the padded inner dimension, thr_T = KMM_CLOSE<T> of agp_cavi.h (1e-3 in fp64, 3e-2 in fp32).
  d2.  The GEMM form adds three inner products of length Dp and two more operations: each term of
      |sx|^2 + |sy|^2 - 2 sx.sy carries at most gamma_{Dp+3} relative to its own magnitude, and |2 sx.sy| <= s2, so
      |fl(d2) - d2| <= 2 gamma_{Dp+3} s2.  The kernel keeps that form only where fl(d2) >= thr_T s2, i.e. there the error is at most
      rho d2 with rho = 2 gamma_{Dp+3} / thr_T.  Below the threshold d2 comes from direct differences: one subtraction, one square
      and a sum of Dp terms, gamma_{Dp+2} d2 -- far inside rho d2.  So |fl(d2) - d2| <= rho d2 for every element.
  value.  First order in that error, plus the roundings of the function evaluation relative to |g|:
      b_ij = variance * ( |dg/dd2| d2 rho + (c0 + |a|) u |g| ) + tiny_T
      g the kernel function, a the argument handed to exp (its rounding error delta enters as |a| delta), dg/dd2 from the
      reference, tiny_T the smallest normal number of T (the exp clamp of fp64 at d2 > 1500 resp. a < -750, whose true values are
      below 1e-325, fp64's gradual underflow, and fp32's flushed denormals).
  c0 collects the function-evaluation roundings, from the bounds the header states:
      fp64: 97 = 81 (exp_nonpos / exp_mhalf: "max relative error ... 9e-15" at the top of agp_cavi.h, 9e-15 / 2^-53 = 81)
                 + 16 (square root, the Matern polynomial -- at most 7 operations on positive terms --, the argument product
                       sqrt(5) * d with its rounded constant, the product with the variance, the variance's own rounding to T)
      fp32: 16 = 1.5 ulp of v_exp_f32 = 3 u, the rounded log2(e) and its product, plus the same handful.
  fp64 squared-exponential STREAMING form (SPEC 1: predict_f without covariance).  It skips the repair by contract ("the GEMM form
      leaves d2 an absolute error of a few ulp(|x|^2 + |y|^2)"): |fl(d2) - d2| <= 2 gamma_{Dp+3} s2 everywhere, and with
      |dg/dd2| = g / 2:   b_ij = variance * g * ( gamma_{Dp+3} s2 + (c0 + |a|) u ) + tiny_T.
The VALU kernel (D > KMM_MAXD = 128, or AGP_KERNELMATRIX_VALU=1) forms direct differences throughout; it is held to the same budget.
"""
import functools

import numpy as np

LD = np.longdouble
KINDS = [("sqexponential", 0), ("matern52", 1), ("matern32", 2), ("exponential", 3)]
NPT = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
TINY = {"f64": float(np.finfo(np.float64).tiny), "f32": float(np.finfo(np.float32).tiny)}
THR = {"f64": 1e-3, "f32": 3e-2}  # KMM_CLOSE<T>, csrc/agp_cavi.h
C0 = {"f64": 97.0, "f32": 16.0}
KMM_MAXD = 128  # csrc/agp_cavi.h


def gamma(k, u):
    return k * u / (1.0 - k * u)


def dp(D):
    return (D + 7) // 8 * 8


def rho(dtype, D):
    return 2.0 * gamma(dp(D) + 3, U[dtype]) / THR[dtype]


def scaled(X, scales, dtype):
    """X[i][d] * T(scale_d), one multiply in T."""
    T = NPT[dtype]
    X = np.asarray(X)
    assert X.dtype == T, "inputs are rounded to T by the caller: the reference sees what the device sees"
    s = np.broadcast_to(np.asarray(scales, dtype=np.float64), (X.shape[1],)).astype(T)
    return np.multiply(X, s, dtype=T)


def distances(sx, sy):
    """(d2, s2) in long double from the scaled rows: direct differences only."""
    sx, sy = sx.astype(LD), sy.astype(LD)
    d2 = np.zeros((len(sx), len(sy)), dtype=LD)
    for d0 in range(0, sx.shape[1], 32):
        df = sx[:, None, d0:d0 + 32] - sy[None, :, d0:d0 + 32]
        d2 += np.sum(df * df, axis=2)
    s2 = np.sum(sx * sx, axis=1)[:, None] + np.sum(sy * sy, axis=1)[None, :]
    return d2, s2


def kernel_fn(kind, d2):
    """(g, a, |dg/dd2| d2) in long double: kernel function, the argument of its exp, the first-order sensitivity to a relative
    error of d2."""
    d2 = np.asarray(d2, dtype=LD)
    r = np.sqrt(d2)
    if kind == 0:
        a = -d2 / 2
        g = np.exp(a)
        return g, a, g * d2 / 2
    if kind == 1:
        s5 = np.sqrt(LD(5))
        a = -s5 * r
        e = np.exp(a)
        return (1 + s5 * r + 5 * d2 / 3) * e, a, LD(5) / 6 * (1 + s5 * r) * e * d2  # dg/dr = -(5/3) r (1 + sqrt5 r) e ; / (2 r)
    if kind == 2:
        s3 = np.sqrt(LD(3))
        a = -s3 * r
        e = np.exp(a)
        return (1 + s3 * r) * e, a, LD(3) / 2 * e * d2  # dg/dr = -3 r e ; / (2 r)
    a = -r
    g = np.exp(a)
    return g, a, g * r / 2  # dg/dd2 = -g / (2 r)


def budget(kind, dtype, D, variance, d2, s2, streaming=False):
    """b_ij of the module docstring.  streaming: the repair-free contract, which only the fp64 squared-exponential SPEC 1 form has."""
    u, g_k = U[dtype], gamma(dp(D) + 3, U[dtype])
    g, a, sens = kernel_fn(kind, d2)
    var = LD(NPT[dtype](variance))
    rnd = (C0[dtype] + np.abs(a)) * u * np.abs(g)
    if streaming:
        assert kind == 0 and dtype == "f64"
        return var * (g * g_k * s2 + rnd) + TINY[dtype]
    return var * (sens * rho(dtype, D) + rnd) + TINY[dtype]


def reference(kind, dtype, variance, d2):
    """variance * g(d2), the variance as the device holds it: rounded to T."""
    return LD(NPT[dtype](variance)) * kernel_fn(kind, d2)[0]


def mean_budget(K, b, alpha, dalpha, mp, dtype):
    """Row-dot sum_j K_ij alpha_j with K_ij within b_ij, alpha_j within dalpha_j, summed in T over mp terms in any order:
    sum_j (|alpha_j| b_ij + |K_ij| dalpha_j) + gamma_{mp+2} sum_j |K_ij alpha_j|."""
    alpha, dalpha = np.abs(alpha.astype(LD)), dalpha.astype(LD)
    return b @ alpha + np.abs(K) @ dalpha + gamma(mp + 2, U[dtype]) * (np.abs(K) @ alpha)


def symv(Kinv, mu, mp, dtype):
    """alpha = Kinv mu in long double and delta alpha_j = gamma_{mp+2} sum_k |Kinv_jk mu_k| (k_symv runs in T)."""
    Kinv, mu = Kinv.astype(LD), mu.astype(LD)
    return Kinv @ mu, gamma(mp + 2, U[dtype]) * (np.abs(Kinv) @ np.abs(mu))


# ---- engineered inputs ---------------------------------------------------------------------------------------------------------------
def ratios(dtype):
    t = THR[dtype]
    return [0.0, 1e-12, 1e-8, 1e-5, 0.1 * t, 0.9 * t, 1.1 * t, 10 * t]


def partner(rng, x, scales, r):
    """A point at d2 = r * 2 |s.x|^2 from x in the scaled space, in a random direction (float64; the caller rounds to T)."""
    v = rng.standard_normal(len(x))
    v /= np.linalg.norm(v)
    sx = x * scales
    return x + v * np.sqrt(r * 2.0 * (sx @ sx)) / scales


@functools.lru_cache(maxsize=None)
def edge_case(dtype, D, c, scale_key, n=130, p=129):
    """X (n x D) = c 1 + U[0,1)^D and Y (p x D): 96 engineered partners of rows of X -- 12 per ratio of ratios(dtype), the rows spread
    over all row tiles, the last (2-row) tile included -- and 33 independent points, in a random column order with a partner in the
    last (1-column) tile.  scale_key: a float, or "ard" (scales 0.05 .. 20 over the dimensions).  Returns (X, Y, scales, info) with X, Y
    in T and info[j] = (row, ratio) for a partner column, None otherwise; ratios are nominal: rounding Y to T moves the smallest
    (in fp32 down to exact duplicates)."""
    T = NPT[dtype]
    rng = np.random.default_rng([D, int(c), 0 if dtype == "f64" else 1, 7])
    scales = np.geomspace(0.05, 20.0, D) if scale_key == "ard" else np.full(D, float(scale_key))
    if scale_key == "ard":
        rng.shuffle(scales)
    X = (c + rng.random((n, D))).astype(T)
    rows = np.round(np.linspace(0, n - 1, 96)).astype(int)  # 0 .. 129: every row tile, both rows of the last
    rs = ratios(dtype)
    cols = rng.permutation(p)
    if cols[0] != p - 1:  # the first partner (ratio 0, row 0) takes the single column of the last column tile
        cols[list(cols).index(p - 1)], cols[0] = cols[0], p - 1
    Y = np.empty((p, D))
    info = [None] * p
    for q in range(96):
        r = rs[q % len(rs)]
        k = int(rows[(q * 37) % 96])  # decorrelate ratio and row
        Y[cols[q]] = partner(rng, X[k].astype(np.float64), scales, r)
        info[cols[q]] = (k, r)
    Y[cols[96:]] = c + rng.random((p - 96, D))
    X.setflags(write=False)
    Y = Y.astype(T)
    Y.setflags(write=False)
    return X, Y, scales, tuple(info)


@functools.lru_cache(maxsize=None)
def edge_distances(dtype, D, c, scale_key):
    """(d2, s2) of edge_case, computed once and shared by the four kernel kinds."""
    X, Y, scales, _ = edge_case(dtype, D, c, scale_key)
    d2, s2 = distances(scaled(X, scales, dtype), scaled(Y, scales, dtype))
    d2.setflags(write=False)
    s2.setflags(write=False)
    return d2, s2


def scale_for(c):
    """1.7 at the origin; 0.05 away from it, which keeps the kernel values of the engineered pairs off 0 and 1."""
    return 1.7 if c == 0 else 0.05


# ---- the three forms of d2 in T (host emulation; tests/test_kmat_budget_host.py) -----------------------------------------------------
def d2_direct_T(sx, sy):
    T = sx.dtype.type
    t = np.zeros((len(sx), len(sy)), dtype=T)
    for d in range(sx.shape[1]):
        df = np.subtract(sx[:, None, d], sy[None, :, d], dtype=T)
        t = np.add(t, np.multiply(df, df, dtype=T), dtype=T)
    return t


def d2_gemm_T(sx, sy, dtype, repair):
    T = sx.dtype.type
    xn = np.sum(np.multiply(sx, sx, dtype=T), axis=1, dtype=T)
    yn = np.sum(np.multiply(sy, sy, dtype=T), axis=1, dtype=T)
    s2 = np.add(xn[:, None], yn[None, :], dtype=T)
    cross = np.matmul(sx, sy.T, dtype=T)
    d2 = np.subtract(s2, np.multiply(T(2), cross, dtype=T), dtype=T)
    if repair:
        close = d2 < np.multiply(T(THR[dtype]), s2, dtype=T)
        d2 = np.where(close, d2_direct_T(sx, sy), d2)
    return d2


def kernel_T(kind, d2, variance):
    """kernel_base of agp_cavi.h with NumPy's exp, every operation in T."""
    T = d2.dtype.type
    d2 = np.maximum(d2, T(0))
    if kind == 0:
        return T(variance) * np.exp(T(-0.5) * d2)
    d = np.sqrt(d2)
    if kind == 1:
        s5 = T(2.23606797749978969641)
        return T(variance) * ((T(1) + s5 * d + T(5) * d2 / T(3)) * np.exp(-s5 * d))
    if kind == 2:
        s3 = T(1.73205080756887729353)
        return T(variance) * ((T(1) + s3 * d) * np.exp(-s3 * d))
    return T(variance) * np.exp(-d)
