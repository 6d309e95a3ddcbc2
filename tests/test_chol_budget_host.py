"""Host checks of tests/_chol_ref.py: the matrix families, the long-double reference, the two comparison values and the budget that
tests/test_gpu_chol_conditioning.py holds the Cholesky building blocks to.  No GPU."""
import numpy as np
import pytest

import _chol_ref as R

CASES = [(f, n, p, dt) for dt in ("f64", "f32") for (f, n, p) in R.accuracy_cases(dt)]
IDS = [R.case_id(*c) for c in CASES]
EPS_LD = float(np.finfo(np.longdouble).eps)


def _representable(A, dtype):
    return np.array_equal(A.astype(R.NPT[dtype]).astype(np.float64), A, equal_nan=True)


@pytest.mark.parametrize("family,n,par,dtype", CASES, ids=IDS)
def test_family_is_deterministic_and_representable(family, n, par, dtype):
    A, A2 = R.FAMILY[family](n, par, dtype), R.FAMILY[family](n, par, dtype)
    assert A is not A2 and np.array_equal(A, A2)
    assert A.dtype == np.float64 and _representable(A, dtype)
    assert np.array_equal(A, A.T)
    B = R.rhs(n, dtype)
    assert B.shape == (R.RHS, n) and _representable(B, dtype) and np.array_equal(B, R.rhs(n, dtype))


def test_graded_is_a_power_of_two_scaling_of_the_suites_matrix():
    for dtype in ("f64", "f32"):
        s = R.GRADE[dtype]
        A, A0 = R.graded(136, s, dtype), R.spd0(136).astype(R.NPT[dtype]).astype(np.float64)
        d = np.sqrt(np.diag(A) / np.diag(A0))
        m, e = np.frexp(d)
        assert np.all(m == 0.5) and (e - 1).min() >= -s and (e - 1).max() <= s and len(set(e)) > s // 2
        assert np.array_equal(A / np.outer(d, d), A0)
        assert np.linalg.cond(A0) < 10 and np.linalg.cond(A) > 1e12


@pytest.mark.parametrize("family,n,par,dtype", CASES, ids=IDS)
def test_reference_and_comparison_values(family, n, par, dtype):
    """eta(L_ref) <= n eps(long double); LAPACK in T and the plain model both succeed (R.case asserts their infos) and land within
    a factor 100 n of u on eta -- they are comparison values, not garbage."""
    c = R.case(family, n, par, dtype)
    e = R.eta(c.A, c.L_ref)
    print(f"{c.id}: eta(L_ref) = {e / EPS_LD:.2f} eps_ld; model / LAPACK in u: " + ", ".join(
        f"{m} {c.model[m] / c.u:.3g} / {c.lapack[m] / c.u:.3g}" for m in R.METRICS))
    assert e <= n * EPS_LD
    for v in (c.model, c.lapack):
        assert all(np.isfinite(v[m]) and v[m] > 0 for m in R.METRICS + ("S",))
        assert v["eta"] <= 100 * n * c.u
    assert abs(c.model_logdet - float(c.logdet_ref)) <= c.budget["logdet"]


@pytest.mark.parametrize("n,r", R.SINGULAR)
def test_singular_family_is_exact_and_fails_at_r_plus_1(n, r):
    B = R.singular_factor(n, r)
    A = R.singular(n, r)
    assert np.array_equal(B, np.rint(B)) and np.array_equal(A, np.rint(A)) and np.array_equal(A, R.singular(n, r))
    assert np.abs(A).max() < 2 ** 20 and np.abs(B).max() <= 2
    assert np.array_equal(np.diag(B[:r]), np.ones(r)) and np.all(np.abs(np.diag(B[:r], -1)) == 1)
    assert np.count_nonzero(B[:r]) == 2 * r - 1
    assert np.array_equal(B.astype(np.float32) @ B.astype(np.float32).T, A)
    # the Cholesky factor of the leading part is B itself, and the 32-block inverses hold 0 and +-1 only
    for o in range(0, r - R.HB + 1, R.HB):
        X = np.linalg.inv(B[o:o + R.HB, o:o + R.HB])
        assert np.array_equal(X, np.rint(X)) and np.abs(X).max() == 1
    if r >= 2:
        assert np.array_equal(np.linalg.cholesky(A[:r, :r]), B[:r])
    assert R.first_bad_pivot(A) == r + 1
    assert R.lapack_potrf(A, "f64")[1] == r + 1
    assert R.lapack_potrf(A, "f32")[1] == r + 1
    with pytest.raises(R.ModelBreakdown):
        R.model(A, "f32")


@pytest.mark.parametrize("i,k", R.NAN_AT)
def test_first_bad_pivot_of_a_nan(i, k):
    # The plain function, not LAPACK, is the reference here: OpenBLAS's potrf was seen to return info 0 on NaN input.
    A = R.with_nan(R.NAN_N, i, k)
    assert np.isnan(A[i, k]) and np.isnan(A[k, i]) and np.isnan(A).sum() == (1 if i == k else 2)
    assert R.first_bad_pivot(A) == i + 1
    assert R.first_bad_pivot(R.spd0(R.NAN_N)) == 0


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("jitter", R.KZZ_JITTER["f64"])
def test_budget_sees_a_degraded_tile_inverse(n, jitter):
    """the plain model with its explicit tile inverses rounded to float32 exceeds the eta and the psi budget on every fp64 kzz case.
    At the smaller jitters the degraded model loses positive definiteness altogether (a Schur complement with a pivot <= 0): the
    device would report that as a failed factorisation, which the GPU test's status assertion catches; it counts as infinite here."""
    c = R.case("kzz", n, jitter, "f64")
    try:
        Ld, Yd, _, _ = R.model(c.A, "f64", c.B, inv_dtype=np.float32)
        got = R.measure(c, Ld, Yd)
    except R.ModelBreakdown:
        got = {"eta": np.inf, "psi": np.inf}
    print(f"{c.id}: eta {got['eta'] / c.u:.3g} u (budget {c.budget['eta'] / c.u:.3g} u), psi {got['psi'] / c.u:.3g} u "
          f"(budget {c.budget['psi'] / c.u:.3g} u)")
    assert got["eta"] > c.budget["eta"] and got["psi"] > c.budget["psi"]


def test_eta_sampled_is_eta_on_its_sample():
    c = R.case("kzz", 328, 1e-4, "f64")
    L = R.model(c.A, "f64")[0]
    LD = R.LD
    res = np.abs(c.A.astype(LD) - L.astype(LD) @ L.astype(LD).T)
    d = np.sqrt(np.diag(c.A).astype(LD))
    res /= np.outer(d, d)
    i, j = R.sample_pairs(328)
    assert len(i) == 328 + 4096 and np.all(i >= j) and np.array_equal(i[:328], np.arange(328)) and np.array_equal(j[:328], i[:328])
    full = float(res[i, j].max())
    got = R.eta_sampled(c.A, L)
    assert abs(got - full) <= 1e-3 * full  # the same entries, summed row-wise instead of by matmul: long-double rounding apart
    assert got <= R.eta(c.A, L)
