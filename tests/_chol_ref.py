"""Ill-conditioned and badly scaled test matrices, an extended-precision reference, error metrics and a plain model of the design's
arithmetic for the Cholesky building blocks (agp_potrf_jitter, agp_spd_inverse, agp_solve_right_spd; csrc/agp_chol.h).  NumPy and
SciPy only; shared by tests/test_chol_budget_host.py (CPU) and tests/test_gpu_chol_conditioning.py (GPU).

T is the type under test (fp64 / fp32), u its unit roundoff (2^-53 / 2^-24).  Every matrix is rounded to T first and kept as fp64;
everything after that -- device, reference, LAPACK, model -- works from those rounded values.  Jitter is added on the host, in T,
and the library is called with jitter = 0.

Families (seeded, deterministic)
    kzz(n, jitter)   squared-exponential kernel, lengthscale 0.5, on default_rng(n).random((n, 2)), plus jitter I: what the library
                     factors first (K_ZZ + jitter I).  fp64: jitter 1e-4, 1e-6, 1e-8 (condition 1e6 .. 1e10); fp32: 1e-2, 1e-3.
    graded(n, s)     D A0 D with A0 = G G' / n + I / 2 (G n x (n + 8), seeded by n: the matrix of tests/test_gpu_tile_rounds.py) rounded
                     to T and D = diag(2^e_i), e_i integers uniform in [-s, s] (s = 100 in fp64, 20 in fp32).  The condition number
                     is huge, the scaled condition below 10; powers of two commute with every operation, so nothing may get worse
                     than on A0.
    singular(n, r)   A = B B', B n x r of integers: the leading r x r block unit lower bidiagonal with subdiagonal +-1, the rows below
                     dense in [-2, 2].  Exactness: B has full column rank and a positive diagonal, so the Cholesky factor of A is B
                     padded with zero columns; the LDL' form has D = I up to column r.  Every quantity an elimination forms before
                     column r -- a pivot (exactly 1), its reciprocal and reciprocal square root (1: the hardware estimates of 1 are
                     1 and a Newton step leaves 1), a multiplier (an entry of B), a partial Schur complement
                     a_ij - sum_{k < c} b_ik b_jk, an entry of a tile inverse (the inverse of a unit bidiagonal +-1 block: 0, +-1)
                     and every partial sum of such integer products in any order -- is an integer below 2^20 < 2^24, so fp32
                     and fp64 compute it without rounding, FMA or not.  Pivot r (0-based) is a_rr - sum_k b_rk^2 = 0 exactly,
                     in any arithmetic order: info = r + 1.
    with_nan(n, i, k) the well-conditioned A0 of size n with A[i, k] = A[k, i] = NaN.  Element (r, c) of a product depends on row r
                     and row c of its operands alone, so the NaN reaches row and column i only and pivot i is the first that is not
                     a positive number: info = i + 1.

Reference (np.longdouble, 64-bit significand): column Cholesky L_ref; X_ref = L_ref^-1 by substitution; A^-1 = X_ref' X_ref;
    logdet = 2 sum log l_ii; B A^-1.  first_bad_pivot(A): the textbook algorithm in fp64, the 1-based index of the first pivot p
    with not (p > 0), 0 if there is none.

Metrics (evaluated in np.longdouble)
    eta(A, L)  = max_ij |A - L L'|_ij / sqrt(a_ii a_jj)      the scaled backward error; needs no reference factor
    eta_sampled           the same over all diagonal entries plus 4096 seeded random pairs i >= j (rows of L gathered in chunks)
    phi(L)     = max_ij |L - L_ref|_ij / sqrt(a_ii)
    psi(Y)     = max_ij |Y - A^-1|_ij / sqrt(A^-1_ii A^-1_jj)
    chi(X)     = ||X - B A^-1||_max / ||B A^-1||_max
    S(L)       = 2 sum_i |l_ii - l_ii^ref| / l_ii^ref        bounds a factor's log-det error and cannot shrink by cancellation

Comparison values, both in T
    LAPACK in T   scipy.linalg.lapack.dpotrf / spotrf, potri, potrs called directly (numpy.linalg.cholesky computes float32 input
                  in double and rounds: 1.8 u where spotrf gives 15 u).
    plain model   the design's arithmetic in NumPy, every operation in T: 64-tiles, each eliminated as two 32-blocks by a
                  hand-written column loop; X11, X22 explicit inverses by substitution; L21 = A21 X11'; S = A22 - L21 L21';
                  panels P1 = T1 X11', P2 = (T2 - P1 L21') X22'; trailing update; X = L^-1 by block substitution from the tile
                  inverses; Y = X' X; logdet = 2 sum log l_ii; B Y.  inv_dtype rounds the explicit tile inverses to a narrower
                  type (the host test's "degraded tile inverse").
                  Two things of csrc/agp_chol.h the model copies, because the first GPU run showed that the explicit inverses
                  do not decide the error on a well-conditioned matrix (graded: eta 13-15 u and phi 8-9 u on the device, all of
                  it on the diagonal, against 3 u and 1.8 u of LAPACK and of a model with neither -- a ratio of 5).  Taken apart
                  on the host at graded(328), the second alone accounts for it (eta 15 u with it, 6 u without); the first
                  changes nothing measurable (15 u against 17 u with exact reciprocals) and is kept so that the model's
                  arithmetic is the device's:
                  * the 32-block elimination is the LDL' form of the device's rounds: raw pivot d, multipliers y rcp1(d),
                    rank-1 updates in place, and L = y rsqrt1(d) at the end, with rcp1 / rsqrt1 the device's estimate-plus-Newton
                    sequences (fp64 rcp1 is one step from a 25-bit estimate: within 19.8 u, measured);
                  * every S = D - L L' (trailing update, the tile's Schur complement, the panel's T2 - P1 L21') starts from the
                    tile and takes the products off one k at a time, as an MFMA accumulator loaded with the tile does: each
                    step rounds at the magnitude of the tile's entry, n roundings of about u a_ii / 2 on a diagonal entry,
                    where a dot product summed from zero and subtracted once per block (LAPACK) rounds at that magnitude n / 64
                    times.  That is a random walk of about sqrt(n) u / 2 on the diagonal residual: it grows with n, not with
                    the conditioning, and stays inside the classic n u.

Budget.  For each metric m of eta, phi, psi, chi: budget = 4 max(m(model), m(LAPACK in T)).  The max keeps a lucky small value of
    either from collapsing the bound.  The factor 4 covers what the model does not copy: the MFMA's order inside a product, the
    hardware estimates' actual bits, Gauss-Jordan in 4-column rounds with a redundant LDL' pivot block instead of a column loop,
    the balanced two-chain form of the task graph's S = D - L L' -- constant factors that depend neither on n nor on the
    conditioning.
    Log-determinant: |ld - ld_ref| <= 4 max(S(model), S(LAPACK)) + 8 * 2^-53 * sum |log l_ii^ref| (the logs and the double sum,
    fp32 included).
    n = 6144 (the blocked driver): eta_sampled(kernel) <= 4 eta_sampled(LAPACK in T); the model is left out (minutes at this size with
    its one-product-at-a-time accumulation; with matrix products instead it took 12-20 s and sat below LAPACK: 16 u against 22 u
    in fp64, 10 u against 31 u in fp32).

Measured
    One MI355X, the run of tests/test_gpu_chol_conditioning.py that came with this file.  In units of u:
    kernel on the default driver (the task graph) / kernel under AGP_CHOL_DAG=0 (k_chol_step, trtri_levels) / plain model / LAPACK in T.
    case                  eta                                   psi                                           chi
    kzz-136-0.0001-f64    23.2 / 22.4 / 21.1 / 7.78             1.64e+05 / 1.38e+05 / 1.31e+05 / 7.92e+04     2.16e+05 / 2.65e+05 / 2.28e+05 / 1.46e+05
    kzz-136-1e-06-f64     166 / 121 / 153 / 7.75                6.10e+07 / 5.01e+07 / 5.56e+07 / 7.95e+06     1.06e+08 / 7.58e+07 / 6.90e+07 / 1.75e+07
    kzz-136-1e-08-f64     597 / 324 / 466 / 7.82                1.58e+10 / 1.06e+10 / 1.04e+10 / 6.77e+08     3.03e+10 / 2.25e+10 / 1.49e+10 / 1.61e+09
    graded-136-100-f64    13.4 / 11.3 / 10.5 / 2.54             15.8 / 12.6 / 14.7 / 5.3                      3.9 / 5.16 / 5.36 / 3.56
    kzz-328-0.0001-f64    87.7 / 87.7 / 70.4 / 14.3             6.12e+05 / 6.04e+05 / 4.37e+05 / 1.42e+05     1.52e+06 / 1.28e+06 / 1.41e+06 / 5.28e+05
    kzz-328-1e-06-f64     579 / 567 / 328 / 15.2                3.82e+08 / 3.44e+08 / 2.56e+08 / 1.36e+07     1.09e+09 / 9.43e+08 / 7.62e+08 / 4.78e+07
    kzz-328-1e-08-f64     1.71e+03 / 1.71e+03 / 1.22e+03 / 15.4  1.24e+11 / 1.22e+11 / 9.89e+10 / 1.28e+09     2.98e+11 / 3.28e+11 / 1.85e+11 / 4.58e+09
    graded-328-100-f64    14.9 / 15.2 / 15 / 2.97               24.1 / 28.7 / 24.7 / 6.81                     10.9 / 8.46 / 10.1 / 4.34
    kzz-136-0.01-f32      6.37 / 7.77 / 10 / 6.32               695 / 689 / 623 / 642                         939 / 1.02e+03 / 1.08e+03 / 1.4e+03
    kzz-136-0.001-f32     12.5 / 13.4 / 11.5 / 6.42             7.65e+03 / 1.04e+04 / 7.51e+03 / 5.87e+03     2.12e+04 / 1.74e+04 / 1.25e+04 / 1.17e+04
    graded-136-20-f32     9.34 / 9.24 / 9.09 / 3.16             11 / 12.8 / 12.1 / 5.68                       9.92 / 7.31 / 5.44 / 4.37
    kzz-328-0.01-f32      12.9 / 13.2 / 14.3 / 14.2             860 / 842 / 1.14e+03 / 1.41e+03               2.94e+03 / 3.11e+03 / 2.76e+03 / 5.58e+03
    kzz-328-0.001-f32     31.6 / 31.6 / 21.2 / 15.1             2.13e+04 / 2.21e+04 / 2.29e+04 / 1.29e+04     6.95e+04 / 7.01e+04 / 5.57e+04 / 4.74e+04
    graded-328-20-f32     13.3 / 15.9 / 15.9 / 3.08             21.2 / 22.2 / 23.9 / 5.57                     18.4 / 19.8 / 21.2 / 4.59
    kzz-6144-0.0001-f64   eta_sampled 12.7 (blocked driver) against LAPACK 21.7
    kzz-6144-0.01-f32     eta_sampled 5.76 (blocked driver) against LAPACK 31.2
    phi sits between 0.6 and 1.8 times max(model, LAPACK) everywhere; the log-determinant uses at most 14 % of its bound.
    Largest kernel / max(model, LAPACK) over all cases, drivers and metrics: 2.03 (chi of kzz-136-1e-08-f64 on the task graph; 1.50
    under AGP_CHOL_DAG=0).  It is the only ratio above 2: that run's A^-1 is already 1.53 times the model's in psi, the solve puts one
    product B A^-1 of 136 terms with cancellation (cond 8e9) on top, and the two drivers, which differ in summation order only,
    are 1.35 apart on it -- the spread of this metric at this conditioning, not one operation.
    Failure reporting: all 40 cases (5 singular, 5 NaN, two types, two drivers) returned status 2 with info = first_bad_pivot from
    agp_potrf_jitter and from agp_spd_inverse.  A^-1 came back symmetric to the bit in every case.
"""
import functools
import types

import numpy as np
from scipy.linalg import lapack

LD = np.longdouble
NPT = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
DT = {"f64": 0, "f32": 1}  # the library's dtype codes
TS, HB = 64, 32  # tile, block of the two-level elimination
RHS = 37  # rows of B in the right solve

KZZ_JITTER = {"f64": (1e-4, 1e-6, 1e-8), "f32": (1e-2, 1e-3)}
GRADE = {"f64": 100, "f32": 20}
SIZES = (136, 328)  # three block columns with 8 valid columns in the last; six block columns
BIG = {"f64": (6144, 1e-4), "f32": (6144, 1e-2)}  # the blocked driver (96 block rows)
SINGULAR = ((192, 5), (192, 32), (192, 64), (192, 100), (200, 130))
NAN_N = 200
NAN_AT = ((5, 5), (40, 3), (70, 10), (130, 64), (199, 0))


def accuracy_cases(dtype):
    """(family, n, parameter) of every accuracy case of the type"""
    out = []
    for n in SIZES:
        out += [("kzz", n, j) for j in KZZ_JITTER[dtype]]
        out.append(("graded", n, GRADE[dtype]))
    return out


def case_id(family, n, par, dtype):
    return f"{family}-{n}-{par:g}-{dtype}"


# ---- families ------------------------------------------------------------------------------------------------------------------------
def _frozen(A):
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def spd0(n):
    """A0 = G G' / n + I / 2, G n x (n + 8), seeded by n (test_gpu_tile_rounds._spd)"""
    G = np.random.default_rng(n).standard_normal((n, n + 8))
    return _frozen(G @ G.T / n + 0.5 * np.eye(n))


def kzz(n, jitter, dtype):
    T = NPT[dtype]
    X = np.random.default_rng(n).random((n, 2))
    d2 = np.zeros((n, n))
    for d in range(2):
        df = X[:, None, d] - X[None, :, d]
        df *= df
        d2 += df
    d2 *= -0.5 / 0.5 ** 2
    A = np.exp(d2, out=d2).astype(T)
    i = np.arange(n)
    A[i, i] = A[i, i] + T(jitter)  # in T
    return _frozen(A.astype(np.float64))


def graded(n, s, dtype):
    T = NPT[dtype]
    e = np.random.default_rng([n, s]).integers(-s, s + 1, n)
    D = np.ldexp(1.0, e)
    A = spd0(n).astype(T).astype(np.float64) * D[:, None] * D[None, :]  # exact: powers of two, far from over- and underflow
    assert np.array_equal(A.astype(T).astype(np.float64), A)
    return _frozen(A)


def singular_factor(n, r):
    rng = np.random.default_rng([n, r])
    B = np.zeros((n, r))
    B[:r] = np.eye(r)
    i = np.arange(1, r)
    B[i, i - 1] = rng.choice([-1.0, 1.0], r - 1)
    B[r:] = rng.integers(-2, 3, (n - r, r))
    return B


def singular(n, r):
    B = singular_factor(n, r)
    return _frozen(B @ B.T)


def with_nan(n, i, k):
    A = spd0(n).copy()
    A[i, k] = A[k, i] = np.nan
    return A


def rhs(n, dtype):
    """the seeded B (RHS x n) of the right solve, rounded to T"""
    return _frozen(np.random.default_rng([n, RHS]).standard_normal((RHS, n)).astype(NPT[dtype]).astype(np.float64))


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def first_bad_pivot(A):
    """textbook column Cholesky in fp64: 1-based index of the first pivot p with not (p > 0), 0 if there is none"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        p = A[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0:
            return j + 1
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0


def chol_ld(A):
    """column Cholesky in long double"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        p = A[j, j] - L[j, :j] @ L[j, :j]
        assert p > 0, (j, p)
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv_ld(L):
    """X = L^-1 by forward substitution in long double"""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = 1 / L[i, i]
    return X


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def eta(A, L):
    A, L = np.asarray(A, dtype=LD), np.asarray(L, dtype=LD)
    d = np.sqrt(np.diag(A))
    return float((np.abs(A - L @ L.T) / np.outer(d, d)).max())


def sample_pairs(n, seed=0, m=4096):
    """(i, j), i >= j: every diagonal entry, then m seeded random pairs"""
    rng = np.random.default_rng([n, seed])
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    i, j = np.maximum(i, j), np.minimum(i, j)
    return np.concatenate([np.arange(n), i]), np.concatenate([np.arange(n), j])


def eta_sampled(A, L, seed=0, chunk=512):
    n = A.shape[0]
    i, j = sample_pairs(n, seed)
    d = np.sqrt(np.diag(A).astype(LD))
    out = 0.0
    for c in range(0, len(i), chunk):
        ii, jj = i[c:c + chunk], j[c:c + chunk]
        r = (L[ii].astype(LD) * L[jj].astype(LD)).sum(axis=1) - A[ii, jj].astype(LD)
        out = max(out, float((np.abs(r) / (d[ii] * d[jj])).max()))
    return out


def phi(A, L, L_ref):
    d = np.sqrt(np.diag(A).astype(LD))
    return float((np.abs(np.asarray(L, dtype=LD) - L_ref) / d[:, None]).max())


def psi(Y, Ainv_ref):
    d = np.sqrt(np.diag(Ainv_ref))
    return float((np.abs(np.asarray(Y, dtype=LD) - Ainv_ref) / np.outer(d, d)).max())


def chi(X, BAinv_ref):
    return float(np.abs(np.asarray(X, dtype=LD) - BAinv_ref).max() / np.abs(BAinv_ref).max())


def s_diag(L, L_ref):
    l, lr = np.diag(np.asarray(L, dtype=LD)), np.diag(L_ref)
    return float(2 * (np.abs(l - lr) / lr).sum())


# ---- comparison values in T ----------------------------------------------------------------------------------------------------------
def lapack_potrf(A, dtype):
    """(L, info) of ?potrf in T; L with a zero strict upper triangle"""
    f = lapack.dpotrf if dtype == "f64" else lapack.spotrf
    c, info = f(np.asarray(A).astype(NPT[dtype]), lower=1, clean=1)
    return c, info


def lapack_all(A, B, dtype):
    """(L, Y = A^-1, X = B A^-1) by ?potrf, ?potri, ?potrs in T"""
    potri, potrs = (lapack.dpotri, lapack.dpotrs) if dtype == "f64" else (lapack.spotri, lapack.spotrs)
    c, info = lapack_potrf(A, dtype)
    assert info == 0, info
    yl, info = potri(c, lower=1)
    assert info == 0, info
    Y = np.tril(yl) + np.tril(yl, -1).T
    xt, info = potrs(c, np.asarray(B).astype(NPT[dtype]).T, lower=1)
    assert info == 0, info
    return c, Y, xt.T


class ModelBreakdown(ArithmeticError):
    pass


def _fma(a, b, c, T):
    """fma(a, b, c) rounded to T once: evaluated in the next wider type (exact for fp32 operands; for fp64 the residual 1 - p r of a
    Newton step keeps 39 of its bits, far more than the step needs)"""
    W = np.float64 if T is np.float32 else LD
    return T(W(a) * W(b) + W(c))


def _estimate(x, T):
    """The hardware estimates (v_rcp / v_rsq).  Measured on an MI355X over 2^20 arguments in [2^-40, 2^40]: the fp64 estimates are
    within 4.7e-8 of the exact value, the fp32 ones within 1.6 u.  Modelled as the exact value rounded to 24 bits (fp64: <= 6e-8)
    and to T (fp32: <= 1 u)."""
    m, e = np.frexp(x)  # the mantissa is rounded, so that an fp64 argument may lie outside fp32's range
    return T(np.ldexp(T(np.float32(m)), e))


def rcp1(p, T):
    """rcp1 of agp_chol.h: estimate and one Newton step.  Measured on an MI355X: within 19.8 u in fp64 (one step squares 4.7e-8),
    1 u in fp32."""
    r = _estimate(1 / LD(p), T)
    return _fma(r, _fma(-p, r, T(1), T), r, T)


def rsqrt1(p, T):
    """rsqrt1 of agp_chol.h: estimate and two (fp64) or one (fp32) Newton steps.  Measured on an MI355X: within 2.2 u and 2.1 u."""
    y = _estimate(1 / np.sqrt(LD(p)), T)
    h = T(0.5) * p
    for _ in range(2 if T is np.float64 else 1):
        y = T(y * _fma(-T(h * y), y, T(1.5), T))
    return y


def _sub_products(C, A, B):
    """C -= A B' the way an MFMA accumulator forms it: the tile is the accumulator's start and the products are taken off one
    k at a time, each step rounded to T at the magnitude of C (a dot product summed from zero and subtracted once rounds at that
    magnitude once per block instead)."""
    for k in range(A.shape[1]):
        C -= np.outer(A[:, k], B[:, k])
    return C


def _chol_block(A, T):
    """The elimination of a block in T, column by column as the device's Gauss-Jordan rounds take it: LDL' form -- raw pivot d_j,
    multipliers f = y rcp1(d_j) from the raw column y, rank-1 update of the trailing block in place -- and L = y rsqrt1(d_j) at the
    end, the diagonal entry d_j rsqrt1(d_j) included (elim_block32 of agp_chol.h).  The lower triangle is read."""
    n = A.shape[0]
    W = np.tril(A).astype(T)
    L = np.zeros((n, n), dtype=T)
    for j in range(n):
        d = W[j, j]
        if not d > 0:
            raise ModelBreakdown(j)
        y = W[j + 1:, j].copy()
        f = y * rcp1(d, T)
        W[j + 1:, j + 1:] -= np.tril(np.outer(f, y))
        rs = rsqrt1(d, T)
        L[j, j] = d * rs
        L[j + 1:, j] = y * rs
    return L


def _inv_block(L, T):
    """explicit inverse of a lower triangular block by forward substitution in T"""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=T)
    for i in range(n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = T(1) / L[i, i]
    return X


def model(A, dtype, B=None, inv_dtype=None):
    """The plain model: (L, Y, logdet, X = B Y); Y, logdet and X only with B.  The matrix is padded to whole tiles with the identity,
    as the library pads it."""
    T = NPT[dtype]
    n = A.shape[0]
    npad = -(-n // TS) * TS
    W = np.eye(npad, dtype=T)
    W[:n, :n] = np.asarray(A).astype(T)
    L = np.zeros((npad, npad), dtype=T)
    Xd = []
    deg = (lambda X: X) if inv_dtype is None else (lambda X: X.astype(inv_dtype).astype(T))
    for k in range(0, npad, TS):
        D = W[k:k + TS, k:k + TS]
        L11 = _chol_block(D[:HB, :HB], T)
        X11 = deg(_inv_block(L11, T))
        L21 = D[HB:, :HB] @ X11.T
        L22 = _chol_block(_sub_products(D[HB:, HB:].copy(), L21, L21), T)
        X22 = deg(_inv_block(L22, T))
        L[k:k + HB, k:k + HB], L[k + HB:k + TS, k:k + HB], L[k + HB:k + TS, k + HB:k + TS] = L11, L21, L22
        Xk = np.zeros((TS, TS), dtype=T)
        Xk[:HB, :HB], Xk[HB:, HB:], Xk[HB:, :HB] = X11, X22, -(X22 @ (L21 @ X11))
        Xd.append(Xk)
        if k + TS < npad:
            Tm = W[k + TS:, k:k + TS]
            P1 = Tm[:, :HB] @ X11.T
            P2 = _sub_products(Tm[:, HB:].copy(), P1, L21) @ X22.T
            P = np.hstack([P1, P2])
            L[k + TS:, k:k + TS] = P
            _sub_products(W[k + TS:, k + TS:], P, P)
    assert L.dtype == T
    if B is None:
        return L[:n, :n].astype(np.float64), None, None, None
    nt = npad // TS
    X = np.zeros((npad, npad), dtype=T)
    t = lambda i, j: (slice(i * TS, (i + 1) * TS), slice(j * TS, (j + 1) * TS))
    for j in range(nt):
        X[t(j, j)] = Xd[j]
        for i in range(j + 1, nt):
            acc = np.zeros((TS, TS), dtype=T)
            for k in range(j, i):
                acc += L[t(i, k)] @ X[t(k, j)]
            X[t(i, j)] = -(Xd[i] @ acc)
    Y = (X.T @ X)[:n, :n]
    logdet = 2.0 * float(np.sum(np.log(np.diag(L)[:n].astype(np.float64))))
    Xs = np.asarray(B).astype(T) @ Y
    assert Y.dtype == T and Xs.dtype == T
    return L[:n, :n].astype(np.float64), Y.astype(np.float64), logdet, Xs.astype(np.float64)


# ---- a case: matrix, reference, comparison values, budgets -----------------------------------------------------------------------------
FAMILY = {"kzz": kzz, "graded": graded}
METRICS = ("eta", "phi", "psi", "chi")


def measure(c, L=None, Y=None, Xs=None):
    """the metrics of whatever is given, against case c"""
    out = {}
    if L is not None:
        out["eta"], out["phi"], out["S"] = eta(c.A, L), phi(c.A, L, c.L_ref), s_diag(L, c.L_ref)
    if Y is not None:
        out["psi"] = psi(Y, c.Ainv_ref)
    if Xs is not None:
        out["chi"] = chi(Xs, c.BAinv_ref)
    return out


@functools.lru_cache(maxsize=None)
def case(family, n, par, dtype):
    """Everything about one accuracy case, computed once and shared: A, B (fp64 arrays of T-representable values, read-only), the
    long-double reference, the metrics of the model and of LAPACK in T, and the budgets."""
    c = types.SimpleNamespace(id=case_id(family, n, par, dtype), family=family, n=n, par=par, dtype=dtype, u=U[dtype])
    c.A, c.B = FAMILY[family](n, par, dtype), rhs(n, dtype)
    c.L_ref = chol_ld(c.A)
    X_ref = tri_inv_ld(c.L_ref)
    c.Ainv_ref = X_ref.T @ X_ref
    logs = np.log(np.diag(c.L_ref))
    c.logdet_ref = 2 * logs.sum()
    c.BAinv_ref = c.B.astype(LD) @ c.Ainv_ref
    Lm, Ym, ldm, Xm = model(c.A, dtype, c.B)
    Ll, Yl, Xl = lapack_all(c.A, c.B, dtype)
    c.model, c.lapack = measure(c, Lm, Ym, Xm), measure(c, Ll, Yl, Xl)
    c.model_logdet = ldm
    c.budget = {m: 4 * max(c.model[m], c.lapack[m]) for m in METRICS}
    c.budget["logdet"] = float(4 * max(c.model["S"], c.lapack["S"]) + 8 * 2.0 ** -53 * np.abs(logs).sum())
    return c


@functools.lru_cache(maxsize=None)
def big_case(dtype):
    """n = 6144: the matrix, LAPACK's factor in T measured by eta_sampled, and the budget 4 eta_sampled(LAPACK)"""
    n, jit = BIG[dtype]
    c = types.SimpleNamespace(id=case_id("kzz", n, jit, dtype), n=n, par=jit, dtype=dtype, u=U[dtype])
    c.A = kzz(n, jit, dtype)
    Ll, info = lapack_potrf(c.A, dtype)
    assert info == 0, info
    c.lapack = {"eta": eta_sampled(c.A, Ll)}
    c.budget = {"eta": 4 * c.lapack["eta"]}
    return c
