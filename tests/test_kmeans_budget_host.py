"""CPU: the per-point budget of tests/_kmeans_ref.py discriminates, and the shift that csrc/agp_kmeans.h applies is what meets it.

The comparison of k_km_assign, |c_j|^2 - 2 x.c_j in T, is emulated in NumPy (one rounding per operation) on uniform [0, 1)^D data
plus a constant offset -- unnormalised features: years, coordinates, time stamps --
  unshifted    about the origin of the coordinate system: the kernel before the shift was introduced;
  shifted      about s = row 0 of the centres: what the kernel does now.
The budget B_i is translation-invariant.  It must (1) pin the label of nearly every point (a budget wider than the runner-up gap
would accept any answer), (2) be broken by the unshifted form at every non-zero offset -- so the GPU test of the same cases,
tests/test_gpu_kmeans_edges.py, would have caught the cancellation -- and (3) hold for the shifted form everywhere.
These are NumPy figures; the device's are measured by the GPU test."""
import numpy as np
import pytest

import _kmeans_ref as KM

CASES = [(dtype, off, shape) for dtype in ("f32", "f64") for off in KM.OFFSETS[dtype] for shape in KM.SHAPES]
# the one non-zero offset at which the unshifted form happens to violate nothing (63 points, 2 centres)
NO_VIOLATION = {("f64", 2.0 ** 20, (63, 2, 15))}


@pytest.mark.parametrize("dtype,off,shape", CASES, ids=[f"{t}-{o:g}-{'x'.join(map(str, s))}" for t, o, s in CASES])
def test_budget_discriminates_and_the_shift_meets_it(dtype, off, shape):
    N, m, D = shape
    X, C = KM.data(N, m, D, off, dtype)
    d2 = KM.distances(X, C)
    B = KM.budget(d2, C, dtype)
    assert np.all(B > 0)
    if m > 1:
        srt = np.sort(d2, axis=1)
        pinned = float(np.mean(srt[:, 1] - srt[:, 0] > B))
        print(f"{dtype} off={off:g} {shape}: runner-up gap > B_i for {pinned:.3f} of the points")
        assert pinned >= 0.9
    lab_u, _ = KM.emulate(X, C, dtype)
    r_u = KM.check_labels(lab_u, d2, B)
    lab_s, mind_s = KM.emulate(X, C, dtype, shift=C[0])
    r_lab, r_mind = KM.check_labels(lab_s, d2, B), KM.check_mind(mind_s, d2, B)
    r_obj = KM.check_objective(float(np.sum(mind_s.astype(np.float64))), d2, B)
    wrong = float(np.mean(d2[np.arange(N), lab_u] - d2.min(axis=1) > B))
    print(f"{dtype} off={off:g} {shape}: excess / B  unshifted {r_u:.3g} ({wrong:.1%} of the points outside)  shifted label {r_lab:.3g}  "
          f"mind {r_mind:.3g}  objective {r_obj:.3g}")
    if off != 0 and m > 1 and (dtype, off, shape) not in NO_VIOLATION:
        assert r_u > 1.0, "the unshifted comparison passes: the GPU test of this case could not see the cancellation"
    assert r_lab <= 1.0 and r_mind <= 1.0 and r_obj <= 1.0


def test_budget_and_reference_are_translation_invariant():
    """Offsets that are exact in T (powers of two, data on a 2^-10 grid): reference and budget do not move at all."""
    rng = np.random.default_rng(3)
    X0 = np.round(rng.random((50, 5)) * 1024) / 1024
    C0 = np.round(rng.random((7, 5)) * 1024) / 1024
    for dtype, off in (("f32", 1024.0), ("f64", 2.0 ** 30)):
        T = KM.NPT[dtype]
        d0, d1 = KM.distances(X0.astype(T), C0.astype(T)), KM.distances((X0 + off).astype(T), (C0 + off).astype(T))
        assert np.array_equal(d0, d1)
        assert np.array_equal(KM.budget(d0, C0.astype(T), dtype), KM.budget(d1, (C0 + off).astype(T), dtype))


def test_reference_is_the_direct_form_of_the_rounded_inputs():
    """A point on a centre gives d2 = 0 exactly; one that differs in the last bit of one coordinate gives that bit's square."""
    for dtype in ("f64", "f32"):
        T = KM.NPT[dtype]
        x = np.array([[1.7e9 if dtype == "f64" else 1024.25, 3.5, 7.125]], dtype=T)
        y = x.copy()
        y[0, 0] = np.nextafter(y[0, 0], T(np.inf))
        d2 = KM.distances(x, np.concatenate([x, y]))
        assert d2[0, 0] == 0 and d2[0, 1] == (KM.LD(y[0, 0]) - KM.LD(x[0, 0])) ** 2 > 0


def test_predicates_catch_what_they_are_for():
    """Each predicate fails on the smallest violation of its kind."""
    dtype = "f64"
    X, C = KM.data(300, 5, 3, 0.0, dtype)
    d2 = KM.distances(X, C)
    B = KM.budget(d2, C, dtype)
    lab = np.argmin(d2, axis=1).astype(np.int32)
    mind = d2.min(axis=1).astype(np.float64)
    assert KM.check_labels(lab, d2, B) == 0 and KM.check_mind(mind, d2, B) <= 1
    bad = lab.copy()
    bad[17] = np.argsort(d2[17])[1]  # the runner-up
    assert KM.check_labels(bad, d2, B) > 1
    bad[17] = 5
    with pytest.raises(AssertionError):
        KM.check_labels(bad, d2, B)
    m2 = mind.copy()
    m2[3] += 3 * float(B[3])
    assert KM.check_mind(m2, d2, B) > 1
    assert KM.check_objective(float(np.sum(mind)), d2, B) <= 1 < KM.check_objective(float(np.sum(mind)) * (1 + 1e-9), d2, B)
    Cn = np.stack([X[lab == j].mean(axis=0) if np.any(lab == j) else C[j] for j in range(5)])
    assert KM.check_centres(Cn, C, X, lab, dtype) <= 1
    Cb = Cn.copy()
    Cb[2, 1] *= 1 + 1e-9
    assert KM.check_centres(Cb, C, X, lab, dtype) > 1
    lab0 = np.where(lab == 4, 0, lab)  # centre 4 emptied: it has to stay, bit for bit
    Cn0 = np.stack([X[lab0 == j].mean(axis=0) if np.any(lab0 == j) else C[j] for j in range(5)])
    assert KM.check_centres(Cn0, C, X, lab0, dtype) <= 1
    Cn0[4, 0] = np.nextafter(Cn0[4, 0], 2.0)
    with pytest.raises(AssertionError):
        KM.check_centres(Cn0, C, X, lab0, dtype)
