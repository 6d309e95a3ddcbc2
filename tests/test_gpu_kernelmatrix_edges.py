"""GPU: the kernel-matrix kernels (csrc/agp_cavi.h) element by element against the long-double reference and the derived budget of
tests/_kmat_ref.py, at the places the rest of the suite does not reach: data away from the origin, (nearly) coincident points on
both sides of the repair threshold KMM_CLOSE<T>, every dimension at which the code changes path, and all four specialisations of
k_kernelmatrix_mma.

agp_kernelmatrix (SPEC 2: store only; the VALU kernel k_kernelmatrix above D = 128 or with AGP_KERNELMATRIX_VALU=1)
    n = 130 rows (three row tiles, the last with 2 rows), p = 129 columns (three column tiles, the last with 1 column),
    X = c 1 + U[0,1)^D; 96 of the columns are engineered partners of rows of X at d2 / s2 in {0, 1e-12, 1e-8, 1e-5, 0.1 thr, 0.9 thr,
    1.1 thr, 10 thr}, 33 are independent (_kmat_ref.edge_case).  D in {1, 7, 8, 9, 56, 57, 64, 127, 128, 129} at c = 10 -- the D tail
    against Dp = ceil(D / 8) 8, element and 16-byte loads, D = 57 the first fp64 tile over 64 KB of LDS, 128 the last MFMA dimension,
    129 the first VALU one --, all three offsets at D in {8, 57, 128, 129}, one ARD case.  Every element within its budget; every pair
    with d2 = 0 exactly T(variance) bit for bit (direct differences give 0, every exp form returns exactly 1 at 0).  Then once with
    repeated, out-of-order idx two-sided, and once in the symmetric form with idx: out[i][j] = k(X[idx[i]], X[j]), the convention
    tests/test_gpu_parity.py::test_kernelmatrix pins.

behind a handle (SPEC 3: symmetric K_ZZ; SPEC 1: streaming row-dot; SPEC 0: row-dot and store)
    SVGP, Gaussian likelihood, no hyper-optimiser, zero prior mean, m = 96 (mp = 128: two column tiles, identity padding), Z with
    8 near-duplicate pairs at 0.1 thr and none exact, two full-batch steps on N = 200 points.  150 test points: 16 exact copies of rows
    of Z, 16 near copies at 1e-8, the rest random.  mu, L and K^-1 are read back; every reference is built from the read-back values,
    so that only the kernel matrix and one dot product are under test:
      K_ZZ     |L L' - (K_ref + jitter I)| <= b_ij + 4 mp u max|K_ref|  (the backward-error bound tests/test_gpu_chain_prefetch.py
               uses for the factorisation);
      means    predict_f without covariance (SPEC 1) and with the diagonal covariance (SPEC 0) against sum_j K_ref[i][j] alpha_j,
               alpha = K^-1 mu in long double, within _kmat_ref.mean_budget; the fp64 squared-exponential streaming form is held to
               its repair-free contract (budget(streaming=True)).
    get_matrix copies the m x m corner of L only: the padded 32 x 32 identity corner is not readable and not checked here.

The mean budgets are wide where K_ZZ is ill-conditioned (delta alpha dominates); emulated on the CPU, the GEMM form without its repair
still breaks them for the Exponential kernel in every case here (15 ... 4e5 times) and for all four kernels at D = 128, c = 1000.

Measured on an MI355X, worst err / budget over all cases of a path (fp64 | fp32, kernels in the order of KINDS):
  agp_kernelmatrix          0.15 0.15 0.15 0.17 | 0.12 0.20 0.16 0.13      with AGP_KERNELMATRIX_VALU=1  0.013 0.14 0.07 0.016 | 0.08 0.20 0.16 0.08
  ... with idx              0.04 0.04 0.04 0.04 | 0.05 0.10 0.15 0.06
  K_ZZ (SPEC 3)             0.10 0.10 0.10 0.09 | 0.020 0.016 0.019 0.016
  streaming mean (SPEC 1)   0.018 0.006 0.006 0.005 | 5e-4 7e-4 1e-3 8e-4
  row-dot + store (SPEC 0)  0.006 0.006 0.006 0.005 | 6e-4 7e-4 1e-3 8e-4
  repair-free fp64 squared-exponential streaming mean at c = 1000: 1.1e-9 ... 2.8e-8 of max |mean| (direct differences: 1e-11 ... 2e-12).
Found by these cases and fixed (agp_cavi.h, exp2_nonpos_f): the fp32 exp was the bare v_exp_f32, which returns 0 where its result
would be a denormal, and the Matern polynomial and the variance multiplied that lost factor -- 73 times the budget for fp32 Matern 3/2
in the ARD case (D = 9, c = 10, d2 / s2 = 2.2e-2, rows of tile 1 against column 28 of tile 0; true value 1.1e-36, device 0), 1.25 times
for the fp32 squared exponential at D = 128 / 129, c = 100 and in the ARD case.  Those cases stay as the regression test.
The tests print the worst ratio and its place for every case."""
import ctypes as C

import numpy as np
import pytest

import _kmat_ref as KR

pytestmark = pytest.mark.gpu

VARIANCE = 1.3
OFFSETS = {"f64": (0, 10, 1000), "f32": (0, 10, 100)}
DIMS_C10 = (1, 7, 8, 9, 56, 57, 64, 127, 128, 129)
DIMS_ALL_C = (8, 57, 128, 129)
DT = {"f64": 0, "f32": 1}


def edge_cases(dtype):
    lo, _, hi = OFFSETS[dtype]
    return ([(D, 10, KR.scale_for(10)) for D in DIMS_C10] + [(D, c, KR.scale_for(c)) for D in DIMS_ALL_C for c in (lo, hi)]
            + [(9, 10, "ard")])


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    yield dict(torch=torch, AGP=AGP, capi=capi, L=L, ctx=ctx)
    L.agp_ctx_destroy(ctx)


def _kmat(env, dtype, kid, scales, X, Y, idx=None):
    """agp_kernelmatrix on T arrays; Y = None: the symmetric form.  Returns the (rows x cols) result as a T array."""
    torch, capi, L, ctx = env["torch"], env["capi"], env["L"], env["ctx"]
    D = X.shape[1]
    d = capi.KernelDesc()
    d.kind, d.variance, d.has_variance, d.has_transform = kid, VARIANCE, 1, 1
    keep = (C.c_double * D)(*[float(s) for s in scales])
    if np.all(scales == scales[0]):
        d.ard, d.scale, d.ard_scales_host = 0, float(scales[0]), None
    else:
        d.ard, d.scale, d.ard_scales_host = 1, 1.0, C.cast(keep, C.POINTER(C.c_double))
    xd = torch.from_numpy(np.array(X)).cuda()  # (a writable copy: the cached cases are read-only)
    yd = None if Y is None else torch.from_numpy(np.array(Y)).cuda()
    idd = None if idx is None else torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
    rows = len(X) if idx is None else len(idx)
    cols = rows if Y is None else len(Y)
    out = torch.full((rows, cols), float("nan"), dtype=xd.dtype, device="cuda")
    st = L.agp_kernelmatrix(ctx, DT[dtype], C.byref(d), xd.data_ptr(), rows, D, None if idd is None else idd.data_ptr(),
                            None if yd is None else yd.data_ptr(), 0 if yd is None else cols, 0 if yd is None else D, D,
                            out.data_ptr(), cols)
    assert st == 0, L.agp_last_error(ctx)
    return out.cpu().numpy()


def _worst(out, ref, b):
    """(worst err / budget, its (i, j), the over-budget mask)"""
    ratio = np.abs(out.astype(KR.LD) - ref) / b
    ratio = np.where(np.isfinite(out), ratio, np.inf)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i, j]), (int(i), int(j)), ratio > 1


def _place(i, j):
    return f"row {i} (tile {i // 64}, local {i % 64}) col {j} (tile {j // 64}, local {j % 64})"


@pytest.mark.parametrize("kname,kid", KR.KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kernelmatrix_edges(env, dtype, kname, kid):
    T = KR.NPT[dtype]
    over, top = [], 0.0
    for D, c, skey in edge_cases(dtype):
        X, Y, scales, info = KR.edge_case(dtype, D, c, skey)
        d2, s2 = KR.edge_distances(dtype, D, c, skey)
        ref, b = KR.reference(kid, dtype, VARIANCE, d2), KR.budget(kid, dtype, D, VARIANCE, d2, s2)
        out = _kmat(env, dtype, kid, scales, X, Y)
        w, (i, j), bad = _worst(out, ref, b)
        top = max(top, w)
        print(f"kernelmatrix {dtype} {kname} D={D} c={c} scale={skey}: worst err / budget {w:.3e} at {_place(i, j)}, "
              f"d2/s2 = {float(d2[i, j] / s2[i, j]):.2e}, partner {info[j]}")
        for i, j in zip(*np.nonzero(bad)):
            over.append((D, c, skey, _place(i, j), f"d2/s2 = {float(d2[i, j] / s2[i, j]):.2e}", f"err/b = {float(abs(out[i, j] - ref[i, j]) / b[i, j]):.2e}"))
        dup = np.asarray(d2 == 0)
        assert dup.sum() >= 12, (D, c, skey)  # the ratio-0 partners at least
        exact = out[dup] == T(VARIANCE)
        assert exact.all(), ("an exact duplicate does not give T(variance) bit for bit", D, c, skey, out[dup][~exact][:4])
    print(f"kernelmatrix {dtype} {kname}: worst err / budget over all cases {top:.3e}")
    assert not over, over[:20]


@pytest.mark.parametrize("kname,kid", KR.KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kernelmatrix_gathered_rows(env, dtype, kname, kid):
    """idx with repeated and out-of-order rows: two-sided, and the symmetric form (y = NULL), where idx gathers the rows only and the
    columns are x[0 .. n).  D = 57 (element loads, a D tail, the large LDS request in fp64) and D = 129 (VALU), c = 10."""
    T = KR.NPT[dtype]
    for D in (57, 129):
        X, Y, scales, _ = KR.edge_case(dtype, D, 10, KR.scale_for(10))
        d2, s2 = KR.edge_distances(dtype, D, 10, KR.scale_for(10))
        n = len(X)
        rng = np.random.default_rng(D)
        idx = np.concatenate([np.arange(n - 1, -1, -3), [5, 5, 5, n - 1, n - 2, 0, 64, 63], rng.integers(0, n, 80)]).astype(np.int64)
        assert len(idx) > 2 * 64 and len(np.unique(idx)) < len(idx)
        out = _kmat(env, dtype, kid, scales, X, Y, idx=idx)
        ref, b = KR.reference(kid, dtype, VARIANCE, d2[idx]), KR.budget(kid, dtype, D, VARIANCE, d2[idx], s2[idx])
        w, (i, j), bad = _worst(out, ref, b)
        print(f"kernelmatrix idx two-sided {dtype} {kname} D={D}: worst err / budget {w:.3e} at {_place(i, j)} (x row {idx[i]})")
        assert not bad.any(), (D, w, _place(i, j))
        assert (out[np.asarray(d2[idx] == 0)] == T(VARIANCE)).all()
        # symmetric form: the rows come from X and from the engineered partners Y, the columns are the first ns rows of [X; Y]
        XY = np.ascontiguousarray(np.vstack([X, Y]))
        ns = n
        idx = np.concatenate([n + np.arange(len(Y) - 1, -1, -2), [3, 3, n, n, ns - 1], rng.integers(0, len(XY), ns)])[:ns].astype(np.int64)
        out = _kmat(env, dtype, kid, scales, XY, None, idx=idx)
        sxy = KR.scaled(XY, scales, dtype)
        d2s, s2s = KR.distances(sxy[idx], sxy[:ns])
        ref, b = KR.reference(kid, dtype, VARIANCE, d2s), KR.budget(kid, dtype, D, VARIANCE, d2s, s2s)
        w, (i, j), bad = _worst(out, ref, b)
        print(f"kernelmatrix idx symmetric {dtype} {kname} D={D}: worst err / budget {w:.3e} at {_place(i, j)} (x row {idx[i]})")
        assert out.shape == (ns, ns) and not bad.any(), (D, w, _place(i, j))
        dup = np.asarray(d2s == 0)
        assert dup.sum() >= 6 and (out[dup] == T(VARIANCE)).all()


# ---- the three specialisations behind a handle ---------------------------------------------------------------------------------------
M, MP, NTRAIN, NTEST = 96, 128, 200, 150


def handle_scale(D, c):
    """Independent points at d2 of order 1 (4 / sqrt(D): E d2 = D s^2 / 6 = 2.7) at c = 10; at c = 1000 a scale that keeps the
    0.1 thr pairs of Z (fp64: d2 = 1e-4 s2, s2 = 2 D c^2 s^2) at d2 of order 1 instead of 1e3: 0.05 sqrt(8 / D)."""
    return 4.0 / np.sqrt(D) if c == 10 else 0.05 * np.sqrt(8.0 / D)


def handle_data(dtype, D, c):
    """Z (with 8 near-duplicate pairs at 0.1 thr), training inputs / targets and the test points, everything already rounded to T
    (held as float64, exactly)."""
    T = KR.NPT[dtype]
    rng = np.random.default_rng([D, int(c), DT[dtype], 11])
    s = np.full(D, handle_scale(D, c))
    Z = c + rng.random((M, D))
    for q in range(8):
        Z[M - 8 + q] = KR.partner(rng, Z[11 * q].astype(T).astype(np.float64), s, 0.1 * KR.THR[dtype])
    Z = Z.astype(T)
    Xtr = (c + rng.random((NTRAIN, D))).astype(T)
    f = np.sin(3 * (Xtr[:, 0].astype(np.float64) - c)) + (Xtr[:, -1].astype(np.float64) - c) ** 2 - 0.7
    y = (f + 0.1 * rng.standard_normal(NTRAIN)).astype(T)
    Xt = c + rng.random((NTEST, D))
    pos = rng.permutation(NTEST)
    for q in range(16):
        Xt[pos[q]] = Z[(5 * q) % M]
        Xt[pos[16 + q]] = KR.partner(rng, Z[(5 * q + 2) % M].astype(np.float64), s, 1e-8)
    return s, Z, Xtr, y, Xt.astype(T), pos


@pytest.mark.parametrize("kname,kid", KR.KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_specialisations_behind_a_handle(env, dtype, kname, kid):
    AGP, capi = env["AGP"], env["capi"]
    T, u = KR.NPT[dtype], KR.U[dtype]
    kcls = {0: AGP.SqExponentialKernel, 1: AGP.Matern52Kernel, 2: AGP.Matern32Kernel, 3: AGP.ExponentialKernel}[kid]
    jitter = KR.LD(T(1e-4 if dtype == "f64" else 1e-3))  # the reference's constant per type, as the device holds it
    over = []
    worst = {"K_ZZ (SPEC 3)": 0.0, "streaming mean (SPEC 1)": 0.0, "row-dot + store mean (SPEC 0)": 0.0}
    for D in (8, 64, 128):
        for c in ((10, 1000) if dtype == "f64" else (10,)):
            s, Z, Xtr, y, Xt, pos = handle_data(dtype, D, c)
            model = AGP.SVGP(VARIANCE * kcls() @ AGP.ScaleTransform(float(s[0])), AGP.GaussianLikelihood(0.01), AGP.AnalyticVI(),
                             Z.astype(np.float64), optimiser=False, T=T)
            AGP.train_(model, Xtr.astype(np.float64), y.astype(np.float64), 2)
            mu = model.get_state(0)[0]
            Lz, Kinv = model.get_matrix(capi.MAT_L), model.get_matrix(capi.MAT_KINV)
            mean1 = AGP.predict_f(model, Xt.astype(np.float64))
            mean0, _ = AGP.predict_f(model, Xt.astype(np.float64), cov=True)
            assert mu.dtype == T and mean1.dtype == T and np.isfinite(mu).all() and np.abs(mu).max() > 0
            tag = (dtype, kname, D, c)
            # K_ZZ: symmetric specialisation, diagonal forced to variance + jitter
            sz = KR.scaled(Z, s, dtype)
            d2, s2 = KR.distances(sz, sz)
            off = ~np.eye(M, dtype=bool)
            assert (np.asarray(d2)[off] > 0).all(), "Z holds no exact duplicates"
            close = np.asarray(d2 < KR.THR[dtype] * s2) & off
            assert close.sum() >= 16, "the 8 near-duplicate pairs (both triangles) sit under the repair threshold"
            Kref, b = KR.reference(kid, dtype, VARIANCE, d2), KR.budget(kid, dtype, D, VARIANCE, d2, s2)
            LL = Lz.astype(KR.LD) @ Lz.astype(KR.LD).T
            assert np.array_equal(Lz, np.tril(Lz))
            bound = b + 4 * MP * u * np.max(np.abs(Kref))
            r = np.abs(LL - (Kref + jitter * np.eye(M, dtype=KR.LD))) / bound
            i, j = np.unravel_index(np.argmax(r), r.shape)
            print(f"handle {tag}: K_ZZ worst err / bound {float(r[i, j]):.3e} at {_place(i, j)}; over the near-duplicate pairs "
                  f"{float(r[close].max()):.3e}")
            worst["K_ZZ (SPEC 3)"] = max(worst["K_ZZ (SPEC 3)"], float(r[i, j]))
            if not r[i, j] <= 1:
                over.append(("K_ZZ", tag, _place(i, j), float(r[i, j])))
            # the two means
            alpha, dalpha = KR.symv(Kinv, mu, MP, dtype)
            d2, s2 = KR.distances(KR.scaled(Xt, s, dtype), sz)
            assert (np.asarray(d2 == 0).sum(axis=1)[pos[:16]] >= 1).all(), "16 test points are exact copies of rows of Z"
            Kref = KR.reference(kid, dtype, VARIANCE, d2)
            want = Kref @ alpha
            stream = dtype == "f64" and kid == 0
            for path, got, bk in (("streaming mean (SPEC 1)", mean1, KR.budget(kid, dtype, D, VARIANCE, d2, s2, streaming=stream)),
                                  ("row-dot + store mean (SPEC 0)", mean0, KR.budget(kid, dtype, D, VARIANCE, d2, s2))):
                bm = KR.mean_budget(Kref, bk, alpha, dalpha, MP, dtype)
                r = np.abs(got.astype(KR.LD) - want) / bm
                r = np.where(np.isfinite(got), r, np.inf)
                i = int(np.argmax(r))
                kindof = "exact copy" if i in pos[:16] else "near copy" if i in pos[16:32] else "random"
                print(f"handle {tag}: {path} worst err / budget {float(r[i]):.3e} at test point {i} ({kindof}, tile {i // 64})")
                worst[path] = max(worst[path], float(r[i]))
                if not r[i] <= 1:
                    over.append((path, tag, i, kindof, float(r[i])))
                if stream and c == 1000 and path.startswith("streaming"):
                    rel = float(np.max(np.abs(got.astype(KR.LD) - want)) / np.max(np.abs(want)))
                    print(f"handle {tag}: repair-free streaming mean, max |err| / max |mean| = {rel:.3e} "
                          f"(budget / max |mean| = {float(np.max(bm) / np.max(np.abs(want))):.3e})")
            del model
    for path, w in worst.items():
        print(f"handle {dtype} {kname}: {path} worst err / budget {w:.3e}")
    assert not over, over
