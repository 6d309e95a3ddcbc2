"""Extended-precision reference and per-point error budget for the k-means selection kernels (csrc/agp_kmeans.h: k_km_assign,
k_km_cnorm, k_km_sums / k_km_finish).  NumPy only; shared by tests/test_kmeans_budget_host.py (CPU) and
tests/test_gpu_kmeans_edges.py (GPU).  LD, U, NPT and gamma are those of tests/_kmat_ref.py.

Reference
    The caller rounds points and centres to T: the reference sees what the device sees.  From those values
    d2[i][j] = sum_d (x_id - c_jd)^2 by direct differences in np.longdouble (`distances`), blocked over rows and over d to bound
    memory, and best_i = min_j d2[i][j].  The GEMM form |x|^2 + |c|^2 - 2 x.c is never used here.

Budget (derived, not measured).  u = unit roundoff of T, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, Lemma 3.1),
Dp = ceil(D / 16) * 16 the padded inner dimension of the assignment kernel, diam^2 = max_jk |c_j - c_k|^2, and

    B_i = 4 gamma_{Dp+4} (diam^2 + max_j d2[i][j]).

  The kernel picks argmin_j of e_ij = |c_j - s|^2 - 2 (x_i - s).(c_j - s): the |x_i - s|^2 that all centres share is dropped from the
  comparison, and s is the origin the arithmetic is carried out about.  Two inner products of length Dp and two more operations
  (the product with 2, the subtraction): each of the two terms carries at most gamma_{Dp+2} relative to the sum of the magnitudes
  of its products, and by Cauchy-Schwarz |(x_i - s).(c_j - s)| summed by magnitudes is at most |x_i - s| |c_j - s|, so
      |fl(e_ij) - e_ij| <= gamma_{Dp+2} (|c_j - s|^2 + 2 |x_i - s| |c_j - s|).
  For any s in the convex hull of the centres |c_j - s|^2 <= diam^2 (the farthest point of a hull from c_j is a vertex) and
  |x_i - s|^2 <= max_j d2[i][j] (likewise from x_i).  With 2ab <= a^2 + b^2,
      |fl(e_ij) - e_ij| <= gamma_{Dp+2} (2 diam^2 + max_j d2[i][j]) <= 2 gamma_{Dp+2} (diam^2 + max_j d2[i][j]).
  The label is wrong by at most the errors of the TWO compared entries (the one chosen, the true minimum): 4 gamma_{Dp+2} (...).
  The shift itself, fl(x - s), is one subtraction in T of nearby values, u |x - s| per coordinate, and the final sum
  |x_i - s|^2 + e (the distance that is returned) is one more operation on top of an inner product of its own: two extra operations,
  gamma_{Dp+2} -> gamma_{Dp+4}.  That gives the constant 4 gamma_{Dp+4}.
  B_i holds only differences of points and centres: it is translation-invariant by construction.  That is the contract -- adding a
  constant to every coordinate of points and centres changes neither the reference nor the budget, so it must not change what
  the kernel may return.  A kernel that forms |c_j|^2 - 2 x.c_j about the origin of the coordinate system has an error relative to
  |x|^2 + |c|^2 instead and breaks B_i as soon as the data lies far from 0 (tests/test_kmeans_budget_host.py shows it).

Predicates (`check_*` return the worst ratio excess / budget; a test asserts <= 1)
  label      0 <= lab_i < m and d2[i][lab_i] - best_i <= B_i
  distance   |mind_i - best_i| <= B_i
  objective  |obj - sum_i best_i| <= sum_i B_i + N 2^-53 sum_i best_i        (the device sums mind in float64, N terms)
  centres    from labels lab, per centre j with n_j > 0 members and per coordinate d:
             |C_jd - mean| <= gamma_{n_j+2} (1/n_j) sum_{i in j} |x_id|, mean and sums in long double -- the standard bound of a sum of
             n_j terms in any order (Higham, section 4.2) with two more operations for the count and the division.  A centre with
             n_j = 0 is bitwise unchanged.

`emulate` is the device's comparison in T on the CPU, one rounding per operation, about the origin (shift=None: the arithmetic before
the shift was introduced) or about a given point.  Only the host test uses it.
"""
import numpy as np

from _kmat_ref import LD, NPT, U, gamma  # noqa: F401  (re-exported)

SHAPES = [(300, 1, 3), (64, 64, 1), (257, 64, 16), (1000, 65, 17), (777, 130, 33), (600, 129, 128), (63, 2, 15), (8193, 65, 3)]
OFFSETS = {"f32": (0.0, 1024.0), "f64": (0.0, 2.0 ** 20, 1.7e9)}


def dp(D):
    return (D + 15) // 16 * 16


def data(N, m, D, off, dtype):
    """The inputs of the near-argmin cases: uniform [0, 1)^D plus a constant offset, rounded to T."""
    T = NPT[dtype]
    rng = np.random.default_rng(N + m)
    X = (rng.random((N, D)) + off).astype(T)
    C = (rng.random((m, D)) + off).astype(T)
    return X, C


def distances(X, C):
    """d2[i][j] in long double by direct differences; blocked over rows and d (at most ~32 MB of temporaries)."""
    X, C = np.asarray(X).astype(LD), np.asarray(C).astype(LD)
    N, D = X.shape
    m = len(C)
    d2 = np.zeros((N, m), dtype=LD)
    rb = max(1, (1 << 21) // (m * 16))
    for r0 in range(0, N, rb):
        for d0 in range(0, D, 16):
            df = X[r0:r0 + rb, None, d0:d0 + 16] - C[None, :, d0:d0 + 16]
            d2[r0:r0 + rb] += np.sum(df * df, axis=2)
    return d2


def diam2(C):
    return distances(C, C).max()


def budget(d2, C, dtype):
    """B_i of the module docstring."""
    D = np.asarray(C).shape[1]
    return 4 * LD(gamma(dp(D) + 4, U[dtype])) * (diam2(C) + d2.max(axis=1))


def check_labels(lab, d2, B):
    """-> worst (d2[i][lab_i] - best_i) / B_i ; raises if a label is outside [0, m)."""
    lab = np.asarray(lab).astype(np.int64)
    assert lab.shape == (len(d2),) and lab.min() >= 0 and lab.max() < d2.shape[1], "label outside [0, m)"
    ex = d2[np.arange(len(d2)), lab] - d2.min(axis=1)
    return float(np.max(ex / B))


def check_mind(mind, d2, B):
    """-> worst |mind_i - best_i| / B_i."""
    mind = np.asarray(mind)
    assert np.isfinite(mind).all()
    return float(np.max(np.abs(mind.astype(LD) - d2.min(axis=1)) / B))


def check_objective(obj, d2, B):
    """-> |obj - sum best| / (sum B + N 2^-53 sum best)."""
    tot = np.sum(d2.min(axis=1))
    return float(abs(LD(obj) - tot) / (np.sum(B) + len(d2) * LD(2.0 ** -53) * tot))


def check_centres(Cnew, Cold, X, lab, dtype):
    """The centre-update predicate against the labels lab.  -> worst |C_jd - mean| / bound over the centres with members;
    raises if a centre without members is not bitwise the old one."""
    Cnew, Cold, lab = np.asarray(Cnew), np.asarray(Cold), np.asarray(lab).astype(np.int64)
    m = len(Cold)
    n = np.bincount(lab, minlength=m)
    XL = np.asarray(X).astype(LD)
    sums, asums = np.zeros(Cold.shape, dtype=LD), np.zeros(Cold.shape, dtype=LD)
    np.add.at(sums, lab, XL)
    np.add.at(asums, lab, np.abs(XL))
    worst = 0.0
    it = np.dtype(Cold.dtype).itemsize
    iv = {4: np.int32, 8: np.int64}[it]
    for j in range(m):
        if n[j] == 0:
            assert np.array_equal(Cnew[j].view(iv), Cold[j].view(iv)), f"centre {j} has no members and moved"
            continue
        bound = LD(gamma(int(n[j]) + 2, U[dtype])) * asums[j] / int(n[j])
        err = np.abs(Cnew[j].astype(LD) - sums[j] / int(n[j]))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, LD(0), err / bound)  # (bound = 0 only where every member's coordinate is 0: then err must be 0)
        worst = max(worst, float(np.max(r)))
    return worst


def emulate(X, C, dtype, shift=None):
    """k_km_cnorm + k_km_assign in T, one rounding per operation, inner products accumulated in d order: (labels, mind).
    shift: the origin s (a row in T) subtracted from points and centres first, or None for the arithmetic about 0."""
    T = NPT[dtype]
    X, C = np.asarray(X), np.asarray(C)
    assert X.dtype == T and C.dtype == T
    if shift is not None:
        s = np.asarray(shift, dtype=T)
        X, C = np.subtract(X, s, dtype=T), np.subtract(C, s, dtype=T)
    cn, xn = np.zeros(len(C), dtype=T), np.zeros(len(X), dtype=T)
    acc = np.zeros((len(X), len(C)), dtype=T)
    for d in range(X.shape[1]):
        cn = np.add(cn, np.multiply(C[:, d], C[:, d], dtype=T), dtype=T)
        xn = np.add(xn, np.multiply(X[:, d], X[:, d], dtype=T), dtype=T)
        acc = np.add(acc, np.multiply(X[:, d, None], C[None, :, d], dtype=T), dtype=T)
    e = np.subtract(cn[None, :], np.multiply(T(2), acc, dtype=T), dtype=T)
    lab = np.argmin(e, axis=1)  # ties -> the smaller index
    mind = np.add(xn, e[np.arange(len(X)), lab], dtype=T)
    return lab.astype(np.int32), np.where(mind < 0, T(0), mind)
