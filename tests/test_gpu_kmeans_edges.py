"""GPU: agp_nearest_center / agp_kmeans (csrc/agp_kmeans.h) against the long-double reference and the per-point budget of
tests/_kmeans_ref.py -- off the unit cube, at the tile / chunk / dimension edges, and through every output.

tests/test_gpu_kmeans.py compares with the float64 oracle on data in [0, 4)^D.  Here the data also lies at a large constant offset
(1024 in fp32, 1.7e9 -- a Unix time stamp -- in fp64), where a comparison of |c|^2 - 2 x.c about the coordinate origin loses
every digit that separates the centres (tests/test_kmeans_budget_host.py), and every assertion is one of the predicates of
tests/_kmeans_ref.py: a returned label is a near-argmin within the translation-invariant budget B_i, the returned distance and
objective are within it, an updated centre is the mean of its members within the bound of a sum in any order.
Shapes: D in {1, 3, 15, 16, 17, 33, 128}; m in {1, 2, 64, 65, 129, 130} (one centre, a full 64-tile, one and two more than a tile);
N in {63, 64, 257, ..., 8193, 16385} (one more than one / two KM_CHUNK = 8192 chunks of the centre sums).
Every printed ratio is excess / budget: <= 1 passes."""
import ctypes as C
import functools

import numpy as np
import pytest

import _kmeans_ref as KM
from _pitched import Pitched

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5  # AGP_ERR_INVALID, AGP_ERR_UNSUPPORTED
DT = {"f64": 0, "f32": 1}
BIG = {"f32": 1024.0, "f64": 1.7e9}  # the large offset of each type
DTYPES = ["f64", "f32"]
CASES = [(dtype, off, shape) for dtype in ("f32", "f64") for off in KM.OFFSETS[dtype] for shape in KM.SHAPES]
LLOYD_SHAPES = [(8193, 65, 3), (16385, 130, 17), (600, 129, 128), (64, 64, 1)]


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    yield dict(torch=torch, L=L, ctx=ctx)
    L.agp_ctx_destroy(ctx)


def _dev(env, a):
    return env["torch"].tensor(np.asarray(a), device="cuda")


def _nearest(env, X, Cc, dtype):
    """agp_nearest_center on contiguous copies -> (labels, mind) as NumPy arrays."""
    torch, L, ctx = env["torch"], env["L"], env["ctx"]
    assert X.dtype == KM.NPT[dtype] and Cc.dtype == KM.NPT[dtype]
    Xd, Cd = _dev(env, X), _dev(env, Cc)
    lab = torch.full((len(X),), -7, dtype=torch.int32, device="cuda")
    md = torch.full((len(X),), -7.0, dtype=Xd.dtype, device="cuda")
    st = L.agp_nearest_center(ctx, DT[dtype], Xd.data_ptr(), len(X), X.shape[1], X.shape[1], Cd.data_ptr(), X.shape[1], len(Cc),
                              lab.data_ptr(), md.data_ptr())
    assert st == 0, L.agp_last_error(ctx)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), md.cpu().numpy()


def _kmeans(env, X, seeds, dtype, max_iter, tol):
    """agp_kmeans with every output requested -> dict(C, lab, cnt, iters, obj, conv)."""
    torch, L, ctx = env["torch"], env["L"], env["ctx"]
    assert X.dtype == KM.NPT[dtype] and seeds.dtype == KM.NPT[dtype]
    N, D = X.shape
    m = len(seeds)
    Xd, Cd = _dev(env, X), _dev(env, seeds)
    lab = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    it, conv, obj = C.c_int32(-7), C.c_int32(-7), C.c_double(-7.0)
    st = L.agp_kmeans(ctx, DT[dtype], Xd.data_ptr(), N, D, D, Cd.data_ptr(), D, m, max_iter, tol, lab.data_ptr(), cnt.data_ptr(),
                      C.byref(it), C.byref(obj), C.byref(conv))
    assert st == 0, L.agp_last_error(ctx)
    torch.cuda.synchronize()
    return dict(C=Cd.cpu().numpy(), lab=lab.cpu().numpy(), cnt=cnt.cpu().numpy(), iters=it.value, obj=obj.value, conv=conv.value)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_run(a, b):
    return (np.array_equal(_bits(a["C"]), _bits(b["C"])) and np.array_equal(a["lab"], b["lab"]) and np.array_equal(a["cnt"], b["cnt"])
            and a["obj"] == b["obj"])


@functools.lru_cache(maxsize=None)
def _case(dtype, off, shape):
    """(X, C, d2, B) of a near-argmin case, computed once."""
    X, Cc = KM.data(*shape, off, dtype)
    d2 = KM.distances(X, Cc)
    out = (X, Cc, d2, KM.budget(d2, Cc, dtype))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _lloyd_data(dtype, off, shape):
    """Uniform data at the offset and m distinct rows of it as seeds."""
    N, m, D = shape
    rng = np.random.default_rng([N, m, D])
    X = (rng.random((N, D)) + off).astype(KM.NPT[dtype])
    seeds = X[rng.choice(N, m, replace=False)].copy()
    X.setflags(write=False)
    seeds.setflags(write=False)
    return X, seeds


# ---- near-argmin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,off,shape", CASES, ids=[f"{t}-{o:g}-{'x'.join(map(str, s))}" for t, o, s in CASES])
def test_nearest_center_is_a_near_argmin(env, dtype, off, shape):
    """The cases of tests/test_kmeans_budget_host.py on the device; m = 1 is the distance pass of the AFK-MC2 seeding."""
    X, Cc, d2, B = _case(dtype, off, shape)
    lab, mind = _nearest(env, X, Cc, dtype)
    r_lab, r_mind = KM.check_labels(lab, d2, B), KM.check_mind(mind, d2, B)
    print(f"\n{dtype} off={off:g} {shape}: label excess / B {r_lab:.3g}   mind error / B {r_mind:.3g}")
    assert r_lab <= 1.0 and r_mind <= 1.0


# ---- points on centres, duplicated centres ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("N,D", [(200, 4), (70, 33)])
def test_points_on_centres_and_duplicates(env, dtype, big, N, D):
    """Centres j and j + 70 coincide (two different 64-wide centre tiles) and the first min(N, m) = 70 points lie on them: the
    distance is 0 within B_i and the label is the smaller index."""
    T, off = KM.NPT[dtype], BIG[dtype] if big else 0.0
    rng = np.random.default_rng([N, D, 11])
    base = (rng.random((70, D)) + off).astype(T)
    Cc = np.concatenate([base, base])
    X = np.concatenate([base, (rng.random((N - 70, D)) + off).astype(T)])
    d2 = KM.distances(X, Cc)
    B = KM.budget(d2, Cc, dtype)
    lab, mind = _nearest(env, X, Cc, dtype)
    assert np.array_equal(lab[:70], np.arange(70))
    assert np.all(mind[:70].astype(KM.LD) <= B[:70])
    assert np.all(lab < 70)  # everywhere: of two coincident centres the smaller index
    r_lab, r_mind = KM.check_labels(lab, d2, B), KM.check_mind(mind, d2, B)
    print(f"\n{dtype} off={off:g} N={N} D={D}: label excess / B {r_lab:.3g}   mind error / B {r_mind:.3g}")
    assert r_lab <= 1.0 and r_mind <= 1.0


# ---- one Lloyd step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("shape", LLOYD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_lloyd_step(env, dtype, big, shape):
    N, m, D = shape
    off = BIG[dtype] if big else 0.0
    X, seeds = _lloyd_data(dtype, off, shape)
    lab0, _ = _nearest(env, X, seeds, dtype)
    run = _kmeans(env, X, seeds, dtype, 1, 0.0)
    assert run["iters"] == 1
    r_c = KM.check_centres(run["C"], seeds, X, lab0, dtype)
    d2 = KM.distances(X, run["C"])  # against the RETURNED centres
    B = KM.budget(d2, run["C"], dtype)
    r_lab, r_obj = KM.check_labels(run["lab"], d2, B), KM.check_objective(run["obj"], d2, B)
    print(f"\n{dtype} off={off:g} {shape}: centre error / bound {r_c:.3g}   label excess / B {r_lab:.3g}   objective error / bound {r_obj:.3g}")
    assert r_c <= 1.0 and r_lab <= 1.0 and r_obj <= 1.0
    assert np.array_equal(run["cnt"], np.bincount(run["lab"], minlength=m))
    assert _same_run(run, _kmeans(env, X, seeds, dtype, 1, 0.0))  # reproducible, bit for bit


# ---- continuation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
def test_continuation_and_convergence(env, dtype, big):
    """Five calls of one iteration, the centres fed back, are one call of five; iters / converged of a run with a tolerance are what
    the objective sequence of single iterations implies."""
    X, seeds = _lloyd_data(dtype, BIG[dtype] if big else 0.0, (2000, 70, 5))
    tol, cap = 1e-3, 100
    objs = [_kmeans(env, X, seeds, dtype, 0, 0.0)["obj"]]
    full = _kmeans(env, X, seeds, dtype, cap, tol)
    cur, step = seeds, None
    for k in range(1, max(full["iters"], 5) + 1):
        step = _kmeans(env, X, cur, dtype, 1, 0.0)
        assert step["iters"] == 1
        cur = step["C"]
        objs.append(step["obj"])
        if k == 5:
            five = _kmeans(env, X, seeds, dtype, 5, 0.0)
            assert five["iters"] == 5 and five["conv"] == 0
            assert np.array_equal(_bits(five["C"]), _bits(step["C"])) and np.array_equal(five["lab"], step["lab"])
            assert five["obj"] == step["obj"]
        if k == full["iters"]:
            assert np.array_equal(_bits(full["C"]), _bits(step["C"])) and np.array_equal(full["lab"], step["lab"])
            assert full["obj"] == step["obj"]
    hits = [k for k in range(1, len(objs)) if abs(objs[k] - objs[k - 1]) < tol]
    want_iters, want_conv = (hits[0], 1) if hits and hits[0] <= cap else (cap, 0)
    print(f"\n{dtype} big={big}: {full['iters']} iterations, converged {full['conv']}, objective {objs[0]:.6g} -> {full['obj']:.6g}")
    assert (full["iters"], full["conv"]) == (want_iters, want_conv)


# ---- emptied clusters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
def test_emptied_clusters_keep_their_centre(env, dtype, big):
    """Centre 70 is a copy of centre 3 (the other centre tile; ties go to 3) and centre 129 lies at +50 in every coordinate: neither
    gets a point, both stay bit for bit, their counts are 0.  Counts and labels are those of the assignment AFTER the update, so
    centre 3 must not move away from its copy (the copy sits on a data row and would collect it): seed 3 is an isolated row, 20
    below the rest in every coordinate, whose cluster is that row alone and whose mean is the row, bit for bit."""
    T, off = KM.NPT[dtype], BIG[dtype] if big else 0.0
    N, m, D = 1000, 130, 3
    rng = np.random.default_rng(41)
    X = (rng.random((N, D)) + off).astype(T)
    pick = rng.choice(N, m - 2, replace=False)
    X[pick[3]] -= T(20)
    rows = X[pick]
    assert len(np.unique(rows, axis=0)) == m - 2
    seeds = np.concatenate([rows[:70], rows[3:4], rows[70:], (rows[:1].astype(np.float64) + 50.0).astype(T)])
    assert seeds.shape == (m, D) and np.array_equal(seeds[70], seeds[3])
    run = _kmeans(env, X, seeds, dtype, 1, 0.0)
    assert np.array_equal(_bits(run["C"][3]), _bits(seeds[3])) and run["cnt"][3] == 1
    for j in (70, 129):
        assert np.array_equal(_bits(run["C"][j]), _bits(seeds[j])), j
        assert run["cnt"][j] == 0 and not np.any(run["lab"] == j), j
    assert int(run["cnt"].sum()) == N and np.array_equal(run["cnt"], np.bincount(run["lab"], minlength=m))
    lab0, _ = _nearest(env, X, seeds, dtype)
    assert not np.any(lab0 == 70) and not np.any(lab0 == 129)
    assert KM.check_centres(run["C"], seeds, X, lab0, dtype) <= 1.0


# ---- max_iter = 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", [False, True])
def test_max_iter_zero_is_one_assignment(env, dtype, big):
    shape = (8193, 65, 3)
    X, seeds = _lloyd_data(dtype, BIG[dtype] if big else 0.0, shape)
    lab, mind = _nearest(env, X, seeds, dtype)
    run = _kmeans(env, X, seeds, dtype, 0, 1e-3)
    assert run["iters"] == 0 and run["conv"] == 0
    assert np.array_equal(_bits(run["C"]), _bits(seeds))
    assert np.array_equal(run["lab"], lab)
    tot = float(np.sum(mind.astype(KM.LD)))
    assert abs(run["obj"] - tot) <= len(X) * 2.0 ** -53 * tot  # a float64 sum of N terms in any order
    assert np.array_equal(run["cnt"], np.bincount(lab, minlength=shape[1]))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_touch_nothing(env, dtype):
    """D = 129, m > n, max_iter < 0: AGP_ERR_INVALID; more than 16384 centres: AGP_ERR_UNSUPPORTED with a message.  All before any
    launch: canary outputs keep their pre-fill, guard bands their sentinel, the centres their bits."""
    L, ctx = env["L"], env["ctx"]
    rng = np.random.default_rng(8)

    def attempt(n, m, D, max_iter, nearest, want):
        x = Pitched(dtype, data=rng.random((n, D)), device="cuda")
        c = Pitched(dtype, data=rng.random((m, D)), device="cuda")
        c0 = c.bits()
        lab, md, cnt = (Pitched("i32", rows=1, width=n, guard=1, device="cuda"), Pitched(dtype, rows=1, width=n, guard=1, device="cuda"),
                        Pitched("i32", rows=1, width=m, guard=1, device="cuda"))
        it, conv, obj = C.c_int32(-7), C.c_int32(-7), C.c_double(-7.0)
        if nearest:
            assert L.agp_nearest_center(ctx, DT[dtype], x.ptr, n, D, D, c.ptr, D, m, lab.ptr, md.ptr) == want, (n, m, D)
        st = L.agp_kmeans(ctx, DT[dtype], x.ptr, n, D, D, c.ptr, D, m, max_iter, 1e-3, lab.ptr, cnt.ptr, C.byref(it), C.byref(obj),
                          C.byref(conv))
        assert st == want, (n, m, D, max_iter, st)
        assert L.agp_ctx_sync(ctx) == 0
        assert all(q.unwritten().all() and q.check() for q in (lab, md, cnt)), (n, m, D, max_iter)
        assert np.array_equal(c.bits(), c0) and c.check() and x.check()
        assert (it.value, conv.value, obj.value) == (-7, -7, -7.0)

    attempt(100, 10, 129, 10, True, INVALID)
    attempt(10, 11, 3, 10, False, INVALID)
    attempt(100, 10, 3, -1, False, INVALID)
    attempt(16385, 16385, 1, 10, False, UNSUPPORTED)
    assert b"16384" in L.agp_last_error(ctx)
    # the context still works
    X, seeds = _lloyd_data(dtype, 0.0, (64, 64, 1))
    assert _kmeans(env, X, seeds, dtype, 1, 0.0)["iters"] == 1


# ---- one non-finite row (agp_nearest_center only) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_row_gets_a_valid_label_and_a_non_finite_distance(env, dtype, bad):
    """The row's label lies in [0, m) -- it would index the bucket kernel's LDS -- and its distance is NaN (not finite for an
    infinity), never 0; every other row, those of its 64-point tile included, is bit for bit what it is without it."""
    X, Cc, _, _ = _case(dtype, KM.OFFSETS[dtype][0], (1000, 65, 17))
    lab0, mind0 = _nearest(env, X, Cc, dtype)
    Xb = X.copy()
    Xb[77, 5] = bad
    lab, mind = _nearest(env, Xb, Cc, dtype)
    assert 0 <= lab[77] < len(Cc)
    assert np.isnan(mind[77]) if np.isnan(bad) else not np.isfinite(mind[77])
    keep = np.arange(len(X)) != 77
    assert np.array_equal(lab[keep], lab0[keep]) and np.array_equal(_bits(mind[keep]), _bits(mind0[keep]))
