"""Greedy conditional-variance selection, host side: the NumPy restatement (tests/_greedy_ref.py) pinned independently of itself,
the margin condition that makes every GPU parity case decidable, and the Python / C declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

import _greedy_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("case", list(G.CASES))
def test_final_trace_equals_the_nystrom_residual_trace(case):
    """tr(K - K_NZ K_ZZ^-1 K_ZN) with a plain Cholesky solve.  Bound: the solve's error per diagonal entry is about
    eps * cond(K_ZZ) * variance with cond(K_ZZ) <= m * variance / smallest pivot (largest eigenvalue <= trace, smallest >= about the
    last Schur complement), summed over N entries."""
    c = G.CASES[case]
    X, res = G.case_result(case)
    assert res["selected"] == c["m"]
    want = G.subset_trace(G.case_kernel(case), X, res["indices"])
    _, pmin = G.margins(res)
    tol = EPS * (c["m"] * c["variance"] / pmin) * c["variance"] * c["N"]
    err = abs(res["trace"][-1] - want)
    print(f"{case}: trace {res['trace'][-1]:.6e}  Cholesky solve {want:.6e}  |diff| {err:.2e}  bound {tol:.2e}")
    assert err <= tol
    assert abs(res["trace"][-1] - np.sum(res["resid"])) == 0.0


@pytest.mark.parametrize("case", list(G.CASES))
def test_structure_of_the_factor(case):
    c = G.CASES[case]
    X, res = G.case_result(case)
    idx, F = res["indices"], res["factor"]
    assert idx[0] == 0  # the first step is an exact tie: the smaller index wins
    assert len(set(idx.tolist())) == c["m"] and idx.min() >= 0 and idx.max() < c["N"]
    Lz = F[idx, :]
    # lower triangular: above the diagonal stand the residual covariances of points chosen EARLIER, zero up to the rounding of the
    # row-dot -- compared with chol(K_ZZ), whose upper triangle is exactly zero, under the same bound as the rest
    want = np.linalg.cholesky(G.case_kernel(case).matrix(X[idx]))
    # same conditioning argument as above: eps * cond(K_ZZ) on entries of size sqrt(variance)
    _, pmin = G.margins(res)
    tol = EPS * (c["m"] * c["variance"] / pmin) * np.sqrt(c["variance"])
    err = np.max(np.abs(Lz - want))
    print(f"{case}: |factor[idx] - chol(Kzz)| {err:.2e}  bound {tol:.2e}")
    assert err <= tol
    assert np.all(np.diff(res["trace"]) <= 0.0)


@pytest.mark.parametrize("case", list(G.CASES))
def test_margin_condition_of_the_parity_cases(case):
    """A condition on the INPUTS, not a tolerance: device and host arithmetic differ by ~1e-12 relative at most, so with every
    argmax decided by >= 1e-6 relative and every pivot >= 1e-6 variance no argmax can flip."""
    c = G.CASES[case]
    _, res = G.case_result(case)
    gap, pmin = G.margins(res)
    print(f"{case}: smallest relative top-two gap {gap:.2e}, smallest pivot {pmin:.2e} ({pmin / c['variance']:.2e} variance)")
    assert res["gaps"][0] == 0.0  # all residuals equal the variance: an exact tie
    assert gap >= G.MIN_GAP
    assert pmin >= G.MIN_PIVOT * c["variance"]


def test_case_table_covers_the_shapes_and_kernels():
    kinds = {c["kind"] for c in G.CASES.values()}
    assert kinds == set(G.KIND_ID)
    assert {1, 3, 33} <= {c["D"] for c in G.CASES.values()}
    assert any(np.ndim(c["scale"]) for c in G.CASES.values())  # ARD
    for c in G.CASES.values():
        assert c["N"] % 64 and c["N"] % 256 and c["m"] > 64 and c["m"] % 64


def test_early_stop_on_tiled_points():
    X = G.tiled_data()
    res = G.greedy(G.Kernel("sqexponential", 2.0, 1.5), X, 64, tol=1e-9)
    k = res["selected"]
    print(f"tiled: selected {k}, last pivots {res['pivots'][k - 3:k]}, largest residual after them {np.max(res['resid']):.2e}")
    assert k == 40
    assert sorted((res["indices"][:k] % 40).tolist()) == list(range(40))
    assert np.all(res["indices"][k:] == -1) and np.all(res["factor"][:, k:] == 0.0) and np.all(res["trace"][k:] == 0.0)
    # unambiguous: the last real pivots are many orders above tol * variance, what is left many orders below
    assert res["pivots"][k - 1] > 1e4 * 1e-9 * 1.5 and np.max(res["resid"]) < 1e-4 * 1e-9 * 1.5


def test_greedy_beats_a_random_subset_on_long_lengthscales():
    """Not a theorem (on short lengthscales the two are equal), but on the first parity case's data and kernel the greedy trace is
    below that of every random subset tried (printed: by what factor); tests/test_gpu_greedy.py asserts the same of the device."""
    X, _ = G.e2e_data()
    assert np.array_equal(X[:300], G.case_data("sqexp_d3"))
    k = G.case_kernel("sqexp_d3")
    tr = G.greedy(k, X, 64)["trace"][-1]
    ratios = []
    for seed in range(5):
        idx = np.sort(np.random.default_rng(seed).choice(X.shape[0], 64, replace=False))
        ratios.append(G.subset_trace(k, X, idx) / tr)
    print(f"trace(RandomSubset(64)) / trace(ConditionalVariance(64)): {np.round(ratios, 2)}")
    assert min(ratios) > 1.0


def test_prefix_property():
    """The first 64 pivots of an m = 130 run are the pivots of an m = 64 run: a step never looks ahead."""
    X, res = G.case_result("sqexp_d3")
    short = G.greedy(G.case_kernel("sqexp_d3"), X, 64)
    assert np.array_equal(short["indices"], res["indices"][:64])


def test_constructor_refusals():
    import agp_amd as AGP

    k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0)
    a = AGP.ConditionalVariance(5, k)
    assert (a.m, a.tol, a.kernel) == (5, 1e-9, k)
    assert AGP.ConditionalVariance(5, k, tol=0.0).tol == 0.0
    with pytest.raises(ValueError, match="positive"):
        AGP.ConditionalVariance(0, k)
    with pytest.raises(ValueError, match="positive"):
        AGP.ConditionalVariance(-3, k)
    with pytest.raises(TypeError, match="Kernel"):
        AGP.ConditionalVariance(5, "sqexponential")
    with pytest.raises(TypeError, match="Kernel"):
        AGP.ConditionalVariance(5, None)
    with pytest.raises(ValueError, match="tol"):
        AGP.ConditionalVariance(5, k, tol=-1e-9)
    with pytest.raises(ValueError, match="tol"):
        AGP.ConditionalVariance(5, k, tol=float("nan"))


def test_symbol_in_header_and_binding():
    from agp_amd import capi

    h = open(os.path.join(ROOT, "include", "agp_hip.h")).read()
    declared = set(re.findall(r"^agp_status (agp_\w+)\(", h, flags=re.M))
    assert "agp_greedy_variance" in declared
    assert "agp_greedy_variance" in capi.SYMBOLS
    assert len(capi.SYMBOLS["agp_greedy_variance"][1]) == 16
    # the header documents the algorithm, the tie rule and the stop rule
    doc = h[h.index("greedy conditional variance"):h.index("agp_status agp_greedy_variance(")]
    for word in ("ties go to the SMALLER index", "stop if", "tol * variance", "AGP_ERR_NOMEM", "AGP_ERR_INVALID"):
        assert word in doc, word
