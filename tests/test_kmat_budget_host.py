"""CPU: the element-wise budget of tests/_kmat_ref.py discriminates.

Three forms of the squared distance are emulated in NumPy in T precision on the engineered inputs of the GPU test (near-coincident
pairs at d2 / s2 from 0 to ten times the repair threshold, data at an offset c from the origin):
  direct       sum of squared differences (the VALU kernel, and the repair branch of the MFMA kernel);
  repaired     the GEMM form |sx|^2 + |sy|^2 - 2 sx.sy with direct differences below KMM_CLOSE<T> s2 (k_kernelmatrix_mma);
  unrepaired   the GEMM form alone -- the kernel with its repair branch removed.
The kernel function is evaluated in T with NumPy's exp.  Direct and repaired must stay inside the budget everywhere; unrepaired
must break it for the Exponential kernel at every (type, D, offset) and for all four kernels at the largest offset -- a budget that
the broken kernel passed would test nothing.  These are NumPy figures: the device's are measured by
tests/test_gpu_kernelmatrix_edges.py."""
import numpy as np
import pytest

import _kmat_ref as KR

DIMS = (1, 8, 57, 128)
OFFSETS = {"f64": (0, 10, 1000), "f32": (0, 10, 100)}
VARIANCE = 1.3


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_budget_discriminates(dtype):
    worst = {"direct": 0.0, "repaired": 0.0}
    for D in DIMS:
        for c in OFFSETS[dtype]:
            X, Y, scales, _ = KR.edge_case(dtype, D, c, KR.scale_for(c))
            sx, sy = KR.scaled(X, scales, dtype), KR.scaled(Y, scales, dtype)
            d2, s2 = KR.edge_distances(dtype, D, c, KR.scale_for(c))
            forms = {"direct": KR.d2_direct_T(sx, sy), "repaired": KR.d2_gemm_T(sx, sy, dtype, True),
                     "unrepaired": KR.d2_gemm_T(sx, sy, dtype, False)}
            for kname, kind in KR.KINDS:
                ref = KR.reference(kind, dtype, VARIANCE, d2)
                b = KR.budget(kind, dtype, D, VARIANCE, d2, s2)
                ratio = {}
                for form, dT in forms.items():
                    err = np.abs(KR.kernel_T(kind, dT, VARIANCE).astype(KR.LD) - ref)
                    ratio[form] = float(np.max(err / b))
                print(f"{dtype} D={D} c={c} {kname}: worst err / budget  direct {ratio['direct']:.2e}  repaired {ratio['repaired']:.2e}  "
                      f"unrepaired {ratio['unrepaired']:.2e}")
                tag = (dtype, D, c, kname)
                assert ratio["direct"] <= 1.0, tag
                assert ratio["repaired"] <= 1.0, tag
                for form in worst:
                    worst[form] = max(worst[form], ratio[form])
                if kname == "exponential" or c == OFFSETS[dtype][-1]:
                    assert ratio["unrepaired"] > 1.0, tag
    print(f"{dtype}: worst direct {worst['direct']:.2e}, worst repaired {worst['repaired']:.2e}")


def test_streaming_budget_holds_the_unrepaired_sqexp():
    """The repair-free contract of the fp64 squared-exponential streaming form: the GEMM form alone stays inside
    variance g (gamma_{Dp+3} s2 + (c0 + |a|) u) + tiny -- and that budget is the wider one exactly where the repair would have run."""
    dtype = "f64"
    for D in DIMS:
        for c in OFFSETS[dtype]:
            X, Y, scales, _ = KR.edge_case(dtype, D, c, KR.scale_for(c))
            sx, sy = KR.scaled(X, scales, dtype), KR.scaled(Y, scales, dtype)
            d2, s2 = KR.edge_distances(dtype, D, c, KR.scale_for(c))
            b = KR.budget(0, dtype, D, VARIANCE, d2, s2, streaming=True)
            wider = b > KR.budget(0, dtype, D, VARIANCE, d2, s2)
            assert np.array_equal(wider, d2 < KR.THR[dtype] * s2)
            err = np.abs(KR.kernel_T(0, KR.d2_gemm_T(sx, sy, dtype, False), VARIANCE).astype(KR.LD) - KR.reference(0, dtype, VARIANCE, d2))
            ratio = float(np.max(err / b))
            print(f"{dtype} D={D} c={c} sqexponential, GEMM form alone against the streaming budget: {ratio:.2e}")
            assert ratio <= 1.0, (dtype, D, c)


def test_reference_is_the_direct_form_of_the_rounded_inputs():
    """The reference scales in T with one multiply and never touches the GEMM form: an exact duplicate gives d2 = 0 and
    g = 1 exactly, and a pair that differs in the last bit of one coordinate gives exactly that bit's square."""
    for dtype in ("f64", "f32"):
        T = KR.NPT[dtype]
        x = np.array([[1000.25, 3.5, 7.125]], dtype=T)
        y = x.copy()
        y[0, 1] = np.nextafter(y[0, 1], T(10))
        s = np.array([0.05, 2.0, 20.0])  # (the perturbed coordinate scales exactly)
        sx, sy = KR.scaled(x, s, dtype), KR.scaled(y, s, dtype)
        assert sx.dtype == T and np.array_equal(sx, x * s.astype(T))
        d2, s2 = KR.distances(sx, sx)
        assert d2[0, 0] == 0 and s2[0, 0] == 2 * np.sum(sx.astype(KR.LD) ** 2)
        for _, kind in KR.KINDS:
            g, a, sens = KR.kernel_fn(kind, d2)
            assert g[0, 0] == 1 and a[0, 0] == 0 and sens[0, 0] == 0
        d2, _ = KR.distances(sx, sy)
        assert d2[0, 0] == (KR.LD(sy[0, 1]) - KR.LD(sx[0, 1])) ** 2 > 0


def test_sensitivities_match_a_finite_difference():
    """|dg/dd2| d2 of kernel_fn against a central difference in long double."""
    d2 = np.array([1e-6, 1e-2, 0.7, 3.0, 40.0], dtype=KR.LD)
    h = d2 * KR.LD(1e-4)
    for _, kind in KR.KINDS:
        fd = np.abs(KR.kernel_fn(kind, d2 + h)[0] - KR.kernel_fn(kind, d2 - h)[0]) / (2 * h) * d2
        assert np.allclose(np.asarray(KR.kernel_fn(kind, d2)[2], dtype=float), np.asarray(fd, dtype=float), rtol=1e-6, atol=0)
