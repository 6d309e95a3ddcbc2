"""GPU: the C ABI (include/agp_hip.h, "Layout") with padded leading dimensions, unaligned bases and guard bands.

Every other test hands the library contiguous tensors, where a leading dimension equals the row width and every base pointer is
the start of an allocation.  Here every call is made twice on identical values -- once contiguous, once PITCHED (tests/_pitched.py:
ld > width, base one element past 16-byte alignment, guard rows around, all padding filled with a NaN sentinel) -- and each case
asserts, without any tolerance:
  (a) the pitched result equals the contiguous one BITWISE: a leading dimension or a base offset enters address arithmetic only,
      and every reduction of the library has a fixed order (test_training_is_bitwise_reproducible relies on the same);
  (b) every guard element of every buffer still holds the sentinel, bit for bit;
  (c) poisoned inputs leave every output finite (implied by (a); reported on its own so that a failure says which one broke);
and, so that two equal wrong answers cannot pass,
  (d) the contiguous result meets the tolerance of the existing test of that entry point (copied from tests/test_gpu_parity.py,
      test_gpu_kmeans.py, test_gpu_mcgp.py; float32 factorisations, which no other test bounds, get the first-order bound
      4 n cond(A) 2^-24 of a Cholesky-based solve).
Layouts per case (tests/_pitched.py, layouts): ld = width + 1 (breaks ld % VEC of the 16-byte vector loads), width + VEC (keeps
them, with padding), round_up(width, 64) + 64; each with off = 0 and off = 1 element.
Refusals: ld = width - 1 must return AGP_ERR_INVALID, touch nothing and leave the context / handle usable.  Those calls use
buffers of the natural full size, so that even a library WITHOUT the check stays inside the allocation: the largest index it could
reach is (rows - 1) * ld + width - 1 < rows * width.
"""
import ctypes as C

import numpy as np
import pytest

from _pitched import Pitched, layouts

pytestmark = pytest.mark.gpu

INVALID = 1  # AGP_ERR_INVALID
KINDS = [("sqexponential", 0), ("matern52", 1), ("matern32", 2), ("exponential", 3)]
NPT = {"f64": np.float64, "f32": np.float32}
DT = {"f64": 0, "f32": 1}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def env(built):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from agp_amd import capi
    from oracle import agp_ref as R

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    yield dict(torch=torch, capi=capi, R=R, L=L, ctx=ctx)
    L.agp_ctx_destroy(ctx)


def _kdesc(capi, kind, variance, scale, ard=None):
    d = capi.KernelDesc()
    d.kind, d.variance, d.has_variance, d.has_transform = kind, variance, 1, 1
    keep = None
    if ard is not None:
        keep = (C.c_double * len(ard))(*ard)
        d.ard, d.scale, d.ard_scales_host = 1, 1.0, C.cast(keep, C.POINTER(C.c_double))
    else:
        d.ard, d.scale, d.ard_scales_host = 0, scale, None
    return d, keep


def _layouts(dtype):
    """[None] (contiguous) + the six pitched layouts, as (kind of ld, off): the ld itself depends on each buffer's width."""
    return [None] + [(k, off) for k in range(3) for off in (0, 1)]


def _mk(dtype, lay, data=None, rows=None, width=None):
    """A Pitched on the GPU in layout `lay` (None: contiguous, still with guard rows around it)."""
    if data is not None:
        d = np.asarray(data)
        width = d.shape[-1] if d.ndim > 1 else d.shape[0]
    if lay is None:
        return Pitched(dtype, data=data, rows=rows, width=width, device="cuda")
    k, off = lay
    ld = [ld for ld, o in layouts(width, dtype) if o == 0][k]
    return Pitched(dtype, data=data, rows=rows, width=width, ld=ld, off=off, device="cuda")


def _vec(dtype, n, data=None):
    """A dense vector (no leading dimension in the ABI) with guards in front of and behind its ends."""
    return Pitched(dtype, data=data, rows=None if data is not None else 1, width=None if data is not None else n, guard=1,
                   device="cuda")


def _same(a, b):
    return np.array_equal(a.bits(), b.bits())


def _finite(*ps):
    return all(np.isfinite(p.window()).all() for p in ps)


def _written(*ps):
    return all(not p.unwritten().any() for p in ps)


def _checks(*ps):
    for p in ps:
        p.check()


# ---- agp_kernelmatrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname,kid", KINDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kernelmatrix_layouts(env, kname, kid, dtype):
    """ldx, ldy, ldo; D = 3 / 11 take the element loads of k_kernelmatrix_mma, D = 8 / 32 its 16-byte loads -- unless ldx % VEC != 0 or
    the base is off alignment, the combinations no contiguous tensor reaches.  Two-sided with a scale and with ARD scales, and the
    symmetric form with gathered rows."""
    capi, R, L, ctx = env["capi"], env["R"], env["L"], env["ctx"]
    n, p, ns = 150, 77, 40
    tol = 1e-12 if dtype == "f64" else 2e-5  # tests/test_gpu_parity.py::test_kernelmatrix
    for D in (3, 8, 11, 32):
        rng = np.random.default_rng(100 + D)
        X, Y = rng.random((n, D)).astype(NPT[dtype]), rng.random((p, D)).astype(NPT[dtype])
        ard = rng.random(D) + 0.5
        idx = rng.choice(n, ns, replace=False).astype(np.int64)
        for form, scale, a in [("scale", 1.7, None), ("ard", 1.0, ard), ("sym+idx", 2.0, None)]:
            kd, keep = _kdesc(capi, kid, 1.3, scale, a)
            sym = form == "sym+idx"
            ref = None
            for lay in _layouts(dtype):
                x = _mk(dtype, lay, data=X)
                y = None if sym else _mk(dtype, lay, data=Y)
                ix = _vec("i64", ns, data=idx) if sym else None
                rows, cols = (ns, ns) if sym else (n, p)
                out = _mk(dtype, lay, rows=rows, width=cols)
                st = L.agp_kernelmatrix(ctx, DT[dtype], C.byref(kd), x.ptr, rows, x.ld, ix.ptr if sym else None,
                                        None if sym else y.ptr, 0 if sym else p, 0 if sym else y.ld, D, out.ptr, out.ld)
                tag = (kname, dtype, D, form, lay)
                assert st == 0, (tag, L.agp_last_error(ctx))
                _checks(out, x, *([ix] if sym else [y]))  # (b)
                assert _written(out), tag
                assert _finite(out), tag  # (c)
                if lay is None:
                    ref = out
                    want = (R.Kernel(kname, 2.0, 1.3).matrix(X[idx].astype(float), X[:ns].astype(float)) if sym else
                            R.Kernel(kname, a if a is not None else scale, 1.3).matrix(X.astype(float), Y.astype(float)))
                    err = _rel(out.window(), want)
                    print(f"kernelmatrix {tag}: rel err {err:.2e}")
                    assert err < tol, tag  # (d)
                else:
                    assert _same(out, ref), tag  # (a)


# ---- agp_potrf_jitter / agp_spd_inverse / agp_solve_right_spd -----------------------------------------------------------------------
def _spd(n, dtype):
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n + 3))
    A = (G @ G.T / n + 0.5 * np.eye(n)).astype(NPT[dtype])  # the matrix of tests/test_gpu_parity.py::test_potrf_and_inverse
    return rng, A


def _tol32(A):
    """float32 has no tolerance in the existing tests: first-order forward bound of a Cholesky factor / Cholesky-based inverse or
    solve, c n cond_2(A) u with u = 2^-24 and c = 4 (Higham, Accuracy and Stability, sections 10.1 and 10.3)."""
    return 4.0 * len(A) * np.linalg.cond(A.astype(float)) * 2.0 ** -24


@pytest.mark.parametrize("n,dtype", [(n, t) for t in ("f64", "f32") for n in (5, 64, 100, 257)] + [(2112, "f64")])
def test_potrf_layouts(env, n, dtype):
    """lda, in place: the factor lands in the n x n window, its strict upper triangle is zero, and beyond column n -- where the
    library's padded 64-grid copy and k_zero_strict_upper(a, lda, n) could reach -- the sentinel is intact.  2112: per-column launches."""
    L, ctx = env["L"], env["ctx"]
    _, A = _spd(n, dtype)
    ref = None
    for lay in _layouts(dtype):
        a = _mk(dtype, lay, data=A)
        info = C.c_int32(-1)
        st = L.agp_potrf_jitter(ctx, DT[dtype], a.ptr, a.ld, n, 1e-4, C.byref(info))
        assert st == 0 and info.value == 0, (lay, L.agp_last_error(ctx))
        a.check()  # (b)
        w = a.window()
        assert np.isfinite(w).all(), lay  # (c)
        assert np.all(np.triu(w, 1) == 0), lay
        if lay is None:
            ref = a
            Lref = np.linalg.cholesky(A.astype(float) + 1e-4 * np.eye(n))
            err = _rel(w, Lref)
            print(f"potrf n={n} {dtype}: rel err {err:.2e}")
            assert err < (1e-11 if dtype == "f64" else _tol32(A))  # (d)
        else:
            assert _same(a, ref), lay  # (a)


@pytest.mark.parametrize("n,dtype", [(n, t) for t in ("f64", "f32") for n in (5, 64, 100, 257)] + [(2112, "f64")])
def test_spd_inverse_layouts(env, n, dtype):
    """lda (input, const: bitwise unchanged afterwards), ldi (output)."""
    L, ctx = env["L"], env["ctx"]
    _, A = _spd(n, dtype)
    ref = None
    for lay in _layouts(dtype):
        a = _mk(dtype, lay, data=A)
        before = a.bits()
        inv = _mk(dtype, lay, rows=n, width=n)
        info, ld = C.c_int32(-1), C.c_double()
        st = L.agp_spd_inverse(ctx, DT[dtype], a.ptr, a.ld, n, inv.ptr, inv.ld, C.byref(ld), C.byref(info))
        assert st == 0 and info.value == 0, (lay, L.agp_last_error(ctx))
        _checks(a, inv)  # (b)
        assert np.array_equal(a.bits(), before), lay
        assert _written(inv) and _finite(inv) and np.isfinite(ld.value), lay  # (c)
        if lay is None:
            ref, ldref = inv, ld.value
            err = _rel(inv.window(), np.linalg.inv(A.astype(float)))
            print(f"spd_inverse n={n} {dtype}: rel err {err:.2e}")
            assert err < (1e-10 if dtype == "f64" else _tol32(A))  # (d)
            sl = np.linalg.slogdet(A.astype(float))[1]
            # logdet = 2 sum_i log L_ii: float32 diagonal entries with relative error <= _tol32 move it by at most 2 n _tol32
            assert abs(ld.value - sl) < (1e-9 * max(1.0, abs(sl)) if dtype == "f64" else 2 * n * _tol32(A))
        else:
            assert _same(inv, ref) and ld.value == ldref, lay  # (a)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [100, 257])
def test_solve_right_spd_layouts(env, n, dtype):
    """lda, ldb, ldx; r on, next to and beyond the 64-grid, and larger than n."""
    L, ctx = env["L"], env["ctx"]
    rng, A = _spd(n, dtype)
    for r in (1, 37, 64, 65, 300):
        Bm = rng.standard_normal((r, n)).astype(NPT[dtype])
        ref = None
        for lay in _layouts(dtype):
            a, b = _mk(dtype, lay, data=A), _mk(dtype, lay, data=Bm)
            x = _mk(dtype, lay, rows=r, width=n)
            info = C.c_int32(-1)
            st = L.agp_solve_right_spd(ctx, DT[dtype], a.ptr, a.ld, n, b.ptr, b.ld, r, x.ptr, x.ld, C.byref(info))
            assert st == 0 and info.value == 0, (r, lay, L.agp_last_error(ctx))
            _checks(a, b, x)  # (b)
            assert _written(x) and _finite(x), (r, lay)  # (c)
            if lay is None:
                ref = x
                err = _rel(x.window(), np.linalg.solve(A.astype(float), Bm.astype(float).T).T)
                print(f"solve_right_spd n={n} r={r} {dtype}: rel err {err:.2e}")
                assert err < (1e-10 if dtype == "f64" else _tol32(A))  # (d)
            else:
                assert _same(x, ref), (r, lay)  # (a)


# ---- agp_nearest_center / agp_kmeans ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [3, 16, 17])
@pytest.mark.parametrize("m", [1, 65])
def test_nearest_center_and_kmeans_layouts(env, dtype, D, m):
    """ldx, ldc (centres: input of agp_nearest_center, in/out of agp_kmeans); labels / counts / mind with guards behind their ends."""
    R, L, ctx = env["R"], env["L"], env["ctx"]
    n = 300
    rng = np.random.default_rng(1000 * m + D)
    cen = rng.random((m, D))  # (the unit cube of tests/test_gpu_kmeans.py::test_nearest_center_matches_oracle, whose atol is copied)
    X = (cen[rng.integers(m, size=n)] + 0.04 * rng.standard_normal((n, D))).astype(NPT[dtype])
    seeds = X[rng.choice(n, m, replace=False)].copy()
    ref = None
    for lay in _layouts(dtype):
        x, c = _mk(dtype, lay, data=X), _mk(dtype, lay, data=seeds)
        lab, md = _vec("i32", n), _vec(dtype, n)
        st = L.agp_nearest_center(ctx, DT[dtype], x.ptr, n, x.ld, D, c.ptr, c.ld, m, lab.ptr, md.ptr)
        assert st == 0, (lay, L.agp_last_error(ctx))
        _checks(x, c, lab, md)  # (b)
        assert _written(lab, md) and _finite(md), lay  # (c)
        # Lloyd iterations from the same seeds: the centres are rewritten in place, m x D elements of them
        ck = _mk(dtype, lay, data=seeds)
        lab2, cnt = _vec("i32", n), _vec("i32", m)
        it, conv, obj = C.c_int32(), C.c_int32(), C.c_double()
        st = L.agp_kmeans(ctx, DT[dtype], x.ptr, n, x.ld, D, ck.ptr, ck.ld, m, 100, 1e-3, lab2.ptr, cnt.ptr, C.byref(it), C.byref(obj),
                          C.byref(conv))
        assert st == 0, (lay, L.agp_last_error(ctx))
        _checks(x, ck, lab2, cnt)  # (b)
        assert _written(lab2) and _finite(ck) and np.isfinite(obj.value), lay  # (c)
        got = (lab, md, ck, lab2, cnt, it.value, conv.value, obj.value)
        if lay is None:
            ref = got
            lr, mr = R.nearest_center(X.astype(float), seeds.astype(float))
            Cr, labr, itr, objr, convr = R.kmeans_lloyd(X.astype(float), seeds.astype(float), tol=1e-3, maxiter=100)
            if dtype == "f64":  # (d) tests/test_gpu_kmeans.py
                assert np.array_equal(lab.window()[0], lr) and np.allclose(md.window()[0], mr, rtol=1e-11, atol=1e-13)
                assert it.value == itr and bool(conv.value) == convr and np.array_equal(lab2.window()[0], labr)
                assert _rel(ck.window(), Cr) < 1e-10 and obj.value == pytest.approx(objr, rel=1e-10)
            else:
                assert np.mean(lab.window()[0] == lr) > 0.99 and np.allclose(md.window()[0], mr, rtol=2e-3, atol=1e-4)
            if it.value > 0:
                assert _written(cnt) and int(cnt.window().sum()) == n
        else:
            for g, w in zip(got[:5], ref[:5]):
                assert _same(g, w), lay  # (a)
            assert got[5:] == ref[5:], lay


# ---- model handles ------------------------------------------------------------------------------------------------------------------
LIK_LOGISTIC, LIK_STUDENTT, LIK_LSM = 1, 2, 3


class Handle:
    """A raw agp_svgp handle: what a ccall client holds."""

    def __init__(self, env, dtype, Z, max_batch, lik, stochastic, kernel=(0, 1.5, 2.0), n_latent=1, p0=0.0, p1=0.0, flags=0, lay=None):
        self.env, self.L, self.dtype = env, env["L"], dtype
        capi = env["capi"]
        self.m, self.D = Z.shape
        d = capi.SvgpDesc()
        d.dtype, d.n_latent, d.latent_offset, d.stochastic = DT[dtype], n_latent, 0, stochastic
        d.m, d.D, d.max_batch = self.m, self.D, max_batch
        d.lik.kind, d.lik.n_class, d.lik.p0, d.lik.p1 = lik, n_latent if lik == LIK_LSM else 1, p0, p1
        d.jitter, d.rm_kappa, d.rm_tau, d.elbo_mode, d.flags = 0.0, 0.51, 1.0, 0, flags
        self.h = C.c_void_p()
        assert self.L.agp_svgp_create(env["ctx"], C.byref(d), C.byref(self.h)) == 0, self.err()
        kd, keep = _kdesc(capi, *kernel)
        self.z = _mk(dtype, lay, data=Z.astype(NPT[dtype]))  # set_Z with ldz
        for l in range(n_latent):
            assert self.L.agp_svgp_set_kernel(self.h, l, C.byref(kd)) == 0
            assert self.L.agp_svgp_set_Z(self.h, l, self.z.ptr, self.z.ld) == 0, self.err()
        self.sync()
        self.z.check()

    def err(self):
        return self.L.agp_last_error(self.env["ctx"])

    def sync(self):
        assert self.L.agp_ctx_sync(self.env["ctx"]) == 0, self.err()

    def ok(self, st):
        assert st == 0, (st, self.err())

    def state(self, l=0):
        """get_state into canaries: mu, Sigma, eta1, eta2 (dense m / m x m, guards behind their ends)."""
        m = self.m
        out = [_vec(self.dtype, m), _vec(self.dtype, m * m), _vec(self.dtype, m), _vec(self.dtype, m * m)]
        self.ok(self.L.agp_svgp_get_state(self.h, l, out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr))
        self.sync()
        _checks(*out)
        assert _written(*out)
        return out

    def close(self):
        self.sync()
        self.L.agp_svgp_destroy(self.h)


def _toy(rng, N, D, m):
    X = rng.random((N, D))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7  # tests/test_gpu_parity.py::_toy
    Z = X[rng.permutation(N)[:m]].copy()
    return X, f, Z


def _kernel_scale(R, dtype, Z, variance=1.5):
    """The inverse lengthscale of the training cases: 2.0, the kernel of tests/test_gpu_parity.py, unless the number format cannot carry
    it at this Z.  K~_i = k_ii + jitt - k_i' K^-1 k_i is about jitt at the inducing points (which are data points here) and is formed
    with a rounding error of about u cond(K + jitt I) variance, u the unit roundoff; the library -- like the reference,
    latentgp.jl:213 -- refuses a step whose K~ is negative.  So the scale is doubled until that error is below a tenth of the jitter
    (1e-4 in float64, 1e-3 in float32).  float64 always keeps 2.0; float32 with 150 inducing points in three dimensions has
    u cond variance = 1e-2 at 2.0, ten times the jitter, and takes 8.0 (7e-5)."""
    u, jitt = (2.0 ** -53, 1e-4) if dtype == "f64" else (2.0 ** -24, 1e-3)
    for scale in (2.0, 4.0, 8.0, 16.0):
        K = R.Kernel("sqexponential", scale, variance).matrix(Z, Z) + jitt * np.eye(len(Z))
        if u * np.linalg.cond(K) * variance < jitt / 10:
            return scale
    raise AssertionError("no kernel scale keeps K~ representable")


def _bits(p):
    return p.bits() if isinstance(p, Pitched) else p


def _assert_same_results(got, ref, tag):
    assert got.keys() == ref.keys()
    for k in ref:
        g, w = _bits(got[k]), _bits(ref[k])
        assert np.array_equal(np.asarray(g), np.asarray(w)), (tag, k)


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("m", [20, 150])
@pytest.mark.parametrize("lik,dtype", [("logistic", "f64"), ("studentt", "f32")])
@pytest.mark.parametrize("full", [False, True])
def test_training_layouts(env, lik, dtype, m, D, full):
    """ldx of cavi_step / step_local / prefetch / elbo / elbo_enqueue and ldz of set_Z / get_Z: 6 steps (minibatches through idx with the
    look-ahead prefetch, or the full batch with idx = NULL), the ELBO after every step, then the posterior, a phase-wise step, the
    hyper-gradient (dZ included) and one hyper step + step -- everything bitwise equal to the contiguous run."""
    R, L = env["R"], env["L"]
    rng = np.random.default_rng(7)
    N, B, iters = 300, 64, 6
    X, f, Z = _toy(rng, N, D, m)
    if lik == "logistic":
        y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)
        likid, p0, p1, lr = LIK_LOGISTIC, 0.0, 0.0, R.LogisticLikelihood()
    else:
        y = f + 0.1 * rng.standard_t(3, N)
        likid, p0, p1, lr = LIK_STUDENTT, 3.0, 1.0, R.StudentTLikelihood(3.0, 1.0)
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(iters + 2)]).astype(np.int64)
    nb = N if full else B
    rho = 1.0 if full else N / B
    Xt, yt = X.astype(NPT[dtype]), y.astype(NPT[dtype])
    Xs = rng.random((50, D))  # test points of the predictive mean after the six steps
    scale = _kernel_scale(R, dtype, Z)

    def run(lay):
        h = Handle(env, dtype, Z, nb, likid, 0 if full else 1, kernel=(0, 1.5, scale), p0=p0, p1=p1, lay=lay)
        x, yv = _mk(dtype, lay, data=Xt), _vec(dtype, N, data=yt)
        ix = [None if full else _vec("i64", B, data=idx[i]) for i in range(iters + 2)]
        ip = [None if full else ix[i].ptr for i in range(iters + 2)]
        res = {}
        for i in range(iters):
            h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, x.ld, yv.ptr, ip[i], nb, rho))
            if not full:
                h.ok(L.agp_svgp_prefetch(h.h, x.ptr, x.ld, ip[i + 1], nb))
            e = C.c_double()
            if i % 2 == 0:
                h.ok(L.agp_svgp_elbo(h.h, x.ptr, x.ld, yv.ptr, ip[i], nb, rho, 0, C.byref(e)))
            else:
                tk, rdy = C.c_int32(-1), C.c_int32()
                h.ok(L.agp_svgp_elbo_enqueue(h.h, x.ptr, x.ld, yv.ptr, ip[i], nb, rho, 0, C.byref(tk)))
                h.ok(L.agp_svgp_elbo_fetch(h.h, tk.value, 1, C.byref(e), C.byref(rdy)))
            res[f"elbo{i}"] = e.value
        res["mu"], res["Sigma"], res["eta1"], res["eta2"] = h.state()
        xs, res["pred"] = _mk(dtype, lay, data=Xs.astype(NPT[dtype])), _vec(dtype, len(Xs))
        h.ok(L.agp_svgp_predict_f(h.h, xs.ptr, xs.ld, len(Xs), res["pred"].ptr, None))
        e = C.c_double()
        h.ok(L.agp_svgp_elbo(h.h, x.ptr, x.ld, yv.ptr, ip[iters], nb, rho, 1, C.byref(e)))  # fresh local variables
        res["elbo_fresh"] = e.value
        # the same step in phases
        h.ok(L.agp_svgp_step_local(h.h, x.ptr, x.ld, yv.ptr, ip[iters], nb, rho))
        h.ok(L.agp_svgp_step_stats(h.h))
        h.ok(L.agp_svgp_step_global(h.h))
        res["mu_p"], res["Sigma_p"], res["eta1_p"], res["eta2_p"] = h.state()
        # hyper-gradient on that minibatch, then one hyper step and a step with the moved kernel and inducing points
        h.ok(L.agp_svgp_hyper_configure(h.h, 1, 0.01, 1, 0.001, 0.9, 0.999, 1e-8))
        dv, ds, dZ = C.c_double(), (C.c_double * D)(), _vec(dtype, m * D)
        h.ok(L.agp_svgp_hypergrad(h.h, 0, C.byref(dv), ds, dZ.ptr))
        h.sync()
        dZ.check()
        assert _written(dZ)
        res["dvar"], res["dscale"], res["dZ"] = dv.value, list(ds), dZ
        h.ok(L.agp_svgp_hyper_step(h.h))
        h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, x.ld, yv.ptr, ip[iters + 1], nb, rho))
        res["mu_h"], res["Sigma_h"], res["eta1_h"], res["eta2_h"] = h.state()
        kv, ks = C.c_double(), (C.c_double * D)()
        h.ok(L.agp_svgp_get_kernel(h.h, 0, C.byref(kv), ks))
        res["kvar"], res["kscale"] = kv.value, list(ks)
        zo = _mk(dtype, lay, rows=m, width=D)  # get_Z with ldz
        h.ok(L.agp_svgp_get_Z(h.h, 0, zo.ptr, zo.ld))
        h.ok(L.agp_svgp_check_status(h.h))
        h.sync()
        res["Z"] = zo
        _checks(zo, x, xs, yv, h.z, res["pred"], *[q for q in ix if q is not None])  # (b)
        assert _written(zo)
        for k, v in res.items():  # (c)
            assert np.isfinite(v.window() if isinstance(v, Pitched) else v).all(), (lay, k)
        h.close()
        return res

    ref = run(None)
    # (d) the contiguous run against the oracle after the six steps: tests/test_gpu_parity.py::test_cavi_trajectory_fp64 (1e-9 on eta,
    # 1e-8 on mu / Sigma and on the predictive mean) and ::test_fp32_mode (jitter 1e-3; predictive mean within 2e-3)
    mr = R.SVGP(R.Kernel("sqexponential", scale, 1.5), lr, Z, stochastic=not full, batchsize=B, jitter=1e-4 if dtype == "f64" else 1e-3)
    mr.train(X, y, iters, idx_stream=None if full else list(idx[:iters]), labels_treated=True)
    g = mr.latents[0]
    errs = [_rel(ref[k].window().reshape(np.shape(w)), w) for k, w in (("eta1", g.eta1), ("eta2", g.eta2), ("mu", g.mu), ("Sigma", g.Sigma),
                                                                        ("pred", mr.predict_f(Xs)[0]))]
    print(f"training {lik} {dtype} m={m} D={D} full={full}: rel err eta1 {errs[0]:.2e} eta2 {errs[1]:.2e} mu {errs[2]:.2e} "
          f"Sigma {errs[3]:.2e} predictive mean {errs[4]:.2e}")
    if dtype == "f64":
        assert errs[0] < 1e-9 and errs[1] < 1e-9 and errs[2] < 1e-8 and errs[3] < 1e-8 and errs[4] < 1e-8
    else:
        assert errs[4] < 2e-3
    for lay in _layouts(dtype)[1:]:
        _assert_same_results(run(lay), ref, lay)  # (a)


def test_vgp_set_Z_with_the_inputs_as_Z(env):
    """VGP (AGP_FLAG_FULL): agp_svgp_set_Z installs the N x D training inputs, with ldz; two steps and the posterior bitwise equal."""
    L, capi = env["L"], env["capi"]
    rng = np.random.default_rng(9)
    N, D = 100, 3
    X, f, _ = _toy(rng, N, D, 1)
    y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)

    def run(lay):
        h = Handle(env, "f64", X, N, LIK_LOGISTIC, 0, flags=capi.FLAG_FULL, lay=lay)
        yv = _vec("f64", N, data=y)
        for _ in range(2):
            h.ok(L.agp_svgp_cavi_step(h.h, None, 0, yv.ptr, None, N, 1.0))
        res = dict(zip(("mu", "Sigma", "eta1", "eta2"), h.state()))
        zo = _mk("f64", lay, rows=N, width=D)
        h.ok(L.agp_svgp_get_Z(h.h, 0, zo.ptr, zo.ld))
        h.sync()
        _checks(zo, yv, h.z)
        assert np.array_equal(zo.window(), X)
        res["Z"] = zo
        assert all(_finite(v) for v in res.values())
        # ldz = D - 1: refused, the installed inputs stay
        assert L.agp_svgp_set_Z(h.h, 0, h.z.ptr, D - 1) == INVALID and L.agp_svgp_get_Z(h.h, 0, zo.ptr, D - 1) == INVALID
        h.ok(L.agp_svgp_get_Z(h.h, 0, zo.ptr, zo.ld))
        h.sync()
        assert np.array_equal(zo.window(), X)
        h.close()
        return res

    ref = run(None)
    for lay in _layouts("f64")[1:]:
        _assert_same_results(run(lay), ref, lay)


def _gh():
    x, w = np.polynomial.hermite.hermgauss(100)  # predictions.jl:4
    n, wt = np.ascontiguousarray(x * np.sqrt(2.0)), np.ascontiguousarray(w / np.sqrt(np.pi))
    return n, wt, n.ctypes.data_as(C.POINTER(C.c_double)), wt.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.parametrize("model", ["logistic", "logisticsoftmax"])
def test_predict_layouts(env, model):
    """ldx of predict_f / predict_f_cov / predict_y / proba_y, and guards behind mu / var / cov / y / out0 / out1 for n_t off the
    64-grid of the prediction workspace."""
    R, L = env["R"], env["L"]
    rng = np.random.default_rng(7)
    N, D, m, B, iters = 300, 3, 20, 64, 4
    X, f, Z = _toy(rng, N, D, m)
    if model == "logistic":
        y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)
        nl, likid, lr, yv = 1, LIK_LOGISTIC, R.LogisticLikelihood(), _vec("f64", N, data=y)
    else:
        y = np.digitize(f, np.quantile(f, [0.33, 0.66]))  # 0-based class index
        nl, likid, lr, yv = 3, LIK_LSM, R.LogisticSoftMaxLikelihood(3), _vec("i32", N, data=y.astype(np.int32))
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(iters)]).astype(np.int64)
    h = Handle(env, "f64", Z, B, likid, 1, n_latent=nl)
    x = _mk("f64", None, data=X)
    ixs = [_vec("i64", B, data=idx[i]) for i in range(iters)]  # (kept: a step's idx may be read by the call that follows it)
    for ix in ixs:
        h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, x.ld, yv.ptr, ix.ptr, B, N / B))
    mr = R.SVGP(R.Kernel("sqexponential", 2.0, 1.5), lr, Z, stochastic=True, batchsize=B)
    mr.train(X, y + 1 if nl == 3 else y, iters, idx_stream=list(idx), labels_treated=nl == 1)
    nodes, weights, pn, pw = _gh()
    for nt in (1, 63, 65, 131):
        Xt = rng.random((nt, D))
        ref = None
        for lay in _layouts("f64"):
            xt = _mk("f64", lay, data=Xt)
            o = dict(mu=_vec("f64", nl * nt), var=_vec("f64", nl * nt), mu_c=_vec("f64", nl * nt), cov=_vec("f64", nl * nt * nt),
                     mu_only=_vec("f64", nl * nt), y=_vec("i32", nt), p0=_vec("f64", nl * nt))
            h.ok(L.agp_svgp_predict_f(h.h, xt.ptr, xt.ld, nt, o["mu"].ptr, o["var"].ptr))
            h.ok(L.agp_svgp_predict_f(h.h, xt.ptr, xt.ld, nt, o["mu_only"].ptr, None))  # the streaming means-only launch
            h.ok(L.agp_svgp_predict_f_cov(h.h, xt.ptr, xt.ld, nt, o["mu_c"].ptr, o["cov"].ptr))
            h.ok(L.agp_svgp_predict_y(h.h, xt.ptr, xt.ld, nt, o["y"].ptr))
            if nl == 1:
                o["p1"] = _vec("f64", nt)
            h.ok(L.agp_svgp_proba_y(h.h, xt.ptr, xt.ld, nt, pn, pw, len(nodes), o["p0"].ptr, o["p1"].ptr if nl == 1 else None))
            h.sync()
            _checks(xt, *o.values())  # (b)
            for k, v in o.items():
                assert _written(v), (nt, lay, k)
                assert _finite(v), (nt, lay, k)  # (c)
            if lay is None:
                ref = o
                mfr, vfr = mr.predict_f(Xt, cov=True)
                mu, var = o["mu"].window().reshape(nl, nt), o["var"].window().reshape(nl, nt)
                for k in range(nl):  # (d) tests/test_gpu_parity.py::test_cavi_trajectory_fp64: means 1e-8, one latent: variances 1e-7
                    assert _rel(mu[k], mfr[k]) < 1e-8 and _rel(o["mu_only"].window().reshape(nl, nt)[k], mfr[k]) < 1e-8, (nt, k)
                    assert _rel(o["mu_c"].window().reshape(nl, nt)[k], mfr[k]) < 1e-8, (nt, k)
                if nl == 1:
                    assert _rel(var[0], vfr[0]) < 1e-7 and _rel(np.diagonal(o["cov"].window().reshape(nt, nt)), vfr[0]) < 1e-7, nt
                pr = mr.proba_y(Xt)
                if nl == 1:
                    assert np.array_equal(o["y"].window()[0] != 0, np.asarray(mr.predict_y(Xt)).astype(bool))
                    assert _rel(o["p0"].window()[0], pr[0]) < 1e-8 and _rel(o["p1"].window()[0], pr[1]) < 1e-6
                else:
                    assert np.array_equal(o["y"].window()[0] + 1, mr.predict_y(Xt))
                    assert _rel(o["p0"].window().reshape(nt, nl), pr) < 1e-8
            else:
                _assert_same_results(o, ref, (nt, lay))  # (a)
    # ldx = D - 1: refused by every predictor, nothing written, the handle still predicts
    nt = 65
    xt = _mk("f64", None, data=rng.random((nt, D)))
    o = [_vec("f64", nl * nt), _vec("f64", nl * nt * nt), _vec("i32", nt)]
    assert L.agp_svgp_predict_f(h.h, xt.ptr, D - 1, nt, o[0].ptr, o[0].ptr) == INVALID
    assert L.agp_svgp_predict_f_cov(h.h, xt.ptr, D - 1, nt, o[0].ptr, o[1].ptr) == INVALID
    assert L.agp_svgp_predict_y(h.h, xt.ptr, D - 1, nt, o[2].ptr) == INVALID
    assert L.agp_svgp_proba_y(h.h, xt.ptr, D - 1, nt, pn, pw, len(nodes), o[0].ptr, o[0].ptr) == INVALID
    h.sync()
    _checks(*o)
    assert all(q.unwritten().all() for q in o)
    h.ok(L.agp_svgp_predict_f(h.h, xt.ptr, xt.ld, nt, o[0].ptr, None))
    h.sync()
    assert _written(o[0]) and _finite(o[0])
    h.close()


def test_get_matrix_and_get_state_layouts(env):
    """agp_svgp_get_matrix with ldo > cols and cap > B after a step with B = 63 (off the 64-grid the library pads the batch to): only
    B rows / B elements are written; agp_svgp_get_state with m = 65."""
    R, L, capi = env["R"], env["L"], env["capi"]
    rng = np.random.default_rng(5)
    N, D, m, B = 300, 3, 65, 63
    X, f, Z = _toy(rng, N, D, m)
    y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)
    idx = rng.choice(N, B, replace=False).astype(np.int64)
    h = Handle(env, "f64", Z, 128, LIK_LOGISTIC, 1)
    x, yv, ix = _mk("f64", None, data=X), _vec("f64", N, data=y), _vec("i64", B, data=idx)
    h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, x.ld, yv.ptr, ix.ptr, B, N / B))
    st0 = h.state()
    st1 = h.state()
    for a, b in zip(st0, st1):
        assert _same(a, b) and _finite(a)
    mats = [(capi.MAT_L, m, m), (capi.MAT_KINV, m, m), (capi.MAT_KNM, B, m), (capi.MAT_KAPPA, B, m)]
    vecs = [capi.VEC_KTILDE, capi.VEC_MEAN_F, capi.VEC_VAR_F, capi.VEC_THETA, capi.VEC_C]
    kern = R.Kernel("sqexponential", 2.0, 1.5)
    for which, rows, cols in mats:
        ref = _mk("f64", None, rows=rows, width=cols)
        h.ok(L.agp_svgp_get_matrix(h.h, 0, which, ref.ptr, cols, rows))
        h.sync()
        ref.check()
        assert _written(ref) and _finite(ref)
        w = ref.window()
        if which == capi.MAT_L:  # (d) single operations: 1e-11 (tests/test_gpu_parity.py)
            assert np.all(np.triu(w, 1) == 0) and _rel(w, np.linalg.cholesky(kern.matrix(Z, Z) + 1e-4 * np.eye(m))) < 1e-11
        elif which == capi.MAT_KNM:
            assert _rel(w, kern.matrix(X[idx], Z)) < 1e-12
        for lay in _layouts("f64")[1:]:
            for cap in (rows, rows + 1, rows + 70):
                out = _mk("f64", lay, rows=cap, width=cols)
                h.ok(L.agp_svgp_get_matrix(h.h, 0, which, out.ptr, out.ld, cap))
                h.sync()
                out.check()  # (b)
                un = out.unwritten()
                assert not un[:rows].any() and un[rows:].all(), (which, lay, cap)  # rows beyond the batch are not touched
                assert np.array_equal(out.bits()[:rows], ref.bits()), (which, lay, cap)  # (a)
        # ldo = cols - 1 and cap = rows - 1: refused, nothing written
        out = _mk("f64", None, rows=rows, width=cols)
        assert L.agp_svgp_get_matrix(h.h, 0, which, out.ptr, cols - 1, rows) == INVALID
        assert L.agp_svgp_get_matrix(h.h, 0, which, out.ptr, cols, rows - 1) == INVALID
        h.sync()
        out.check()
        assert out.unwritten().all()
    for which in vecs:
        ref = _vec("f64", B)
        h.ok(L.agp_svgp_get_matrix(h.h, 0, which, ref.ptr, 1, B))
        h.sync()
        ref.check()
        assert _written(ref) and _finite(ref)
        for cap in (B + 1, 128, 200):
            out = _vec("f64", cap)
            h.ok(L.agp_svgp_get_matrix(h.h, 0, which, out.ptr, 1, cap))
            h.sync()
            out.check()
            un = out.unwritten()[0]
            assert not un[:B].any() and un[B:].all(), (which, cap)
            assert np.array_equal(out.bits()[0, :B], ref.bits()[0]), (which, cap)
        out = _vec("f64", B)
        assert L.agp_svgp_get_matrix(h.h, 0, which, out.ptr, 1, B - 1) == INVALID
        h.sync()
        assert out.unwritten().all() and out.check()
    st2 = h.state()  # the handle works afterwards and nothing of it moved
    for a, b in zip(st0, st2):
        assert _same(a, b)
    h.close()


def test_gibbs_store_layouts(env):
    """lds of agp_svgp_gibbs_sample (the store of kept samples) and of agp_svgp_predict_samples, ldx of the latter: one 20-sweep chain
    with N = 100, every kept sample and every prediction bitwise equal to the contiguous chain."""
    import _mcgp_ref as M

    R, L, capi = env["R"], env["L"], env["capi"]
    rng = np.random.default_rng(21)
    N, D, S, nt, seed = 100, 3, 20, 65, 1234
    X, f, _ = _toy(rng, N, D, 1)
    y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)
    Xt = rng.random((nt, D))

    def run(lay):
        h = Handle(env, "f64", X, N, LIK_LOGISTIC, 0, flags=capi.FLAG_FULL | capi.FLAG_SAMPLED, lay=lay)
        yv, store, xt = _vec("f64", N, data=y), _mk("f64", lay, rows=S, width=N), _mk("f64", lay, data=Xt)
        h.ok(L.agp_svgp_gibbs_sample(h.h, yv.ptr, S, 0, 1, C.c_uint64(seed), store.ptr, store.ld))
        h.ok(L.agp_svgp_check_status(h.h))
        res = dict(store=store)
        for mode in (0, 1, 2):
            res[f"o0_{mode}"], res[f"o1_{mode}"] = _vec("f64", nt), _vec("f64", nt)
            h.ok(L.agp_svgp_predict_samples(h.h, xt.ptr, xt.ld, nt, store.ptr, store.ld, S, mode, res[f"o0_{mode}"].ptr,
                                            res[f"o1_{mode}"].ptr if mode else None))
        h.sync()
        _checks(yv, xt, h.z, *res.values())  # (b)
        assert res.pop("o1_0").unwritten().all()
        assert all(_written(v) and _finite(v) for v in res.values()), lay  # (c)
        # lds = N - 1 / ldx = D - 1: refused, nothing written, the chain's counter has not moved
        s2, o2 = _mk("f64", None, rows=S, width=N), _vec("f64", nt)
        assert L.agp_svgp_gibbs_sample(h.h, yv.ptr, S, 0, 1, C.c_uint64(seed), s2.ptr, N - 1) == INVALID
        assert L.agp_svgp_predict_samples(h.h, xt.ptr, xt.ld, nt, store.ptr, N - 1, S, 0, o2.ptr, None) == INVALID
        assert L.agp_svgp_predict_samples(h.h, xt.ptr, D - 1, nt, store.ptr, store.ld, S, 0, o2.ptr, None) == INVALID
        t = C.c_int64(-1)
        h.ok(L.agp_svgp_gibbs_counter(h.h, 0, C.byref(t)))
        h.sync()
        assert t.value == S and s2.unwritten().all() and o2.unwritten().all() and s2.check() and o2.check()
        h.close()
        return res

    ref = run(None)
    mref = M.MCGPRef(R.Kernel("sqexponential", 2.0, 1.5), R.LogisticLikelihood(), X, y, seed)
    Sr = mref.sample(S)
    assert _rel(ref["store"].window(), Sr) < 1e-8  # (d) tests/test_gpu_mcgp.py CHAIN_TOL
    mu_r, var_r = mref.predict_f(Xt, Sr)
    assert _rel(ref["o0_1"].window()[0], mu_r) < 1e-8 and _rel(ref["o1_1"].window()[0], var_r) < 1e-6
    for lay in _layouts("f64")[1:]:
        _assert_same_results(run(lay), ref, lay)  # (a)


def test_online_handover_layouts(env):
    """ldi of agp_svgp_online_snapshot / agp_svgp_set_online_prior and ldza of the latter: one hand-over between two handles (the
    sequence of online.py: snapshot, prior on a handle with more inducing points, first step under the old ones, two more steps)."""
    L = env["L"]
    rng = np.random.default_rng(17)
    N, D, m1, m2, B = 120, 2, 20, 25, 60
    X, f, Z1 = _toy(rng, N, D, m1)
    Z2 = np.concatenate([Z1, rng.random((m2 - m1, D))])
    y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)

    def run(lay):
        old = Handle(env, "f64", Z1, B, LIK_LOGISTIC, 0, lay=lay)
        eye, zero = _mk("f64", lay, data=np.eye(m1)), _vec("f64", m1, data=np.zeros(m1))
        old.ok(L.agp_svgp_set_online_prior(old.h, 0, None, 0, m1, eye.ptr, eye.ld, zero.ptr, 0.0))  # first batch: Z_a empty
        x1, y1 = _mk("f64", lay, data=X[:B]), _vec("f64", B, data=y[:B])
        for _ in range(3):
            old.ok(L.agp_svgp_cavi_step(old.h, x1.ptr, x1.ld, y1.ptr, None, B, 1.0))
        iD, e1, pl = _mk("f64", lay, rows=m1, width=m1), _vec("f64", m1), C.c_double()
        old.ok(L.agp_svgp_online_snapshot(old.h, 0, iD.ptr, iD.ld, e1.ptr, C.byref(pl)))
        _checks(iD, e1, eye, zero)
        assert _written(iD, e1)
        # ldi = m - 1: refused, nothing written
        iD2, e2 = _mk("f64", None, rows=m1, width=m1), _vec("f64", m1)
        assert L.agp_svgp_online_snapshot(old.h, 0, iD2.ptr, m1 - 1, e2.ptr, C.byref(C.c_double())) == INVALID
        old.sync()
        assert iD2.unwritten().all() and e2.unwritten().all() and iD2.check() and e2.check()
        so = old.state()
        kinv = _mk("f64", None, rows=m1, width=m1)
        old.ok(L.agp_svgp_get_matrix(old.h, 0, 1, kinv.ptr, m1, m1))
        old.sync()
        # (d) save_old_gp! (onlinetraining.jl:170-180): invD_a = -2 eta2 - inv(K), from the handle's own exports
        assert _rel(iD.window(), -2.0 * so[3].window().reshape(m1, m1) - kinv.window()) < 1e-10
        new = Handle(env, "f64", Z2, B, LIK_LOGISTIC, 0, lay=lay)
        assert L.agp_svgp_set_online_prior(new.h, 0, old.z.ptr, D - 1, m1, iD.ptr, iD.ld, e1.ptr, pl.value) == INVALID
        assert L.agp_svgp_set_online_prior(new.h, 0, old.z.ptr, old.z.ld, m1, iD.ptr, m1 - 1, e1.ptr, pl.value) == INVALID
        new.ok(L.agp_svgp_set_online_prior(new.h, 0, old.z.ptr, old.z.ld, m1, iD.ptr, iD.ld, e1.ptr, pl.value))
        x2, y2 = _mk("f64", lay, data=X[B:]), _vec("f64", B, data=y[B:])
        assert L.agp_svgp_online_first_step(new.h, old.h, x2.ptr, D - 1, y2.ptr, B) == INVALID
        new.ok(L.agp_svgp_online_first_step(new.h, old.h, x2.ptr, x2.ld, y2.ptr, B))
        for _ in range(2):
            new.ok(L.agp_svgp_cavi_step(new.h, x2.ptr, x2.ld, y2.ptr, None, B, 1.0))
        e = C.c_double()
        new.ok(L.agp_svgp_elbo(new.h, x2.ptr, x2.ld, y2.ptr, None, B, 1.0, 0, C.byref(e)))
        res = dict(zip(("mu", "Sigma", "eta1", "eta2"), new.state()))
        res.update(invDa=iD, eta1_a=e1, prevLa=pl.value, elbo=e.value)
        _checks(x1, y1, x2, y2, iD, e1, old.z, new.z)  # (b)
        for k, v in res.items():  # (c)
            assert np.isfinite(v.window() if isinstance(v, Pitched) else v).all(), (lay, k)
        old.close()
        new.close()
        return res

    ref = run(None)
    for lay in _layouts("f64")[1:]:
        _assert_same_results(run(lay), ref, lay)  # (a)


# ---- refusals of the building blocks and of the training entry points ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kernelmatrix_refuses_small_leading_dimensions(env, dtype):
    """ldx < D, ldy < D, ldo < p (ldo < n in the symmetric form) and p <= 0 with y: AGP_ERR_INVALID, the output untouched, and the
    context computes the same matrix afterwards.  Full-size buffers: an unchecked call stays inside them."""
    capi, L, ctx = env["capi"], env["L"], env["ctx"]
    rng = np.random.default_rng(3)
    n, p, D = 150, 77, 11
    X, Y = rng.random((n, D)), rng.random((p, D))
    kd, _ = _kdesc(capi, 0, 1.3, 1.7)
    x, y = _mk(dtype, None, data=X), _mk(dtype, None, data=Y)
    good = _mk(dtype, None, rows=n, width=p)
    assert L.agp_kernelmatrix(ctx, DT[dtype], C.byref(kd), x.ptr, n, D, None, y.ptr, p, D, D, good.ptr, p) == 0
    bad = [("ldx", dict(ldx=D - 1)), ("ldy", dict(ldy=D - 1)), ("ldo", dict(ldo=p - 1)), ("p = 0", dict(p=0)), ("p < 0", dict(p=-1))]
    for name, kw in bad:
        a = dict(ldx=D, ldy=D, ldo=p, p=p)
        a.update(kw)
        out = _mk(dtype, None, rows=n, width=p)
        st = L.agp_kernelmatrix(ctx, DT[dtype], C.byref(kd), x.ptr, n, a["ldx"], None, y.ptr, a["p"], a["ldy"], D, out.ptr, a["ldo"])
        assert L.agp_ctx_sync(ctx) == 0
        assert st == INVALID, (name, st)
        assert out.unwritten().all() and out.check(), name
    for name, ldx, ldo in [("sym ldx", D - 1, n), ("sym ldo", D, n - 1)]:
        out = _mk(dtype, None, rows=n, width=n)
        st = L.agp_kernelmatrix(ctx, DT[dtype], C.byref(kd), x.ptr, n, ldx, None, None, 0, 0, D, out.ptr, ldo)
        assert L.agp_ctx_sync(ctx) == 0
        assert st == INVALID, (name, st)
        assert out.unwritten().all() and out.check(), name
    again = _mk(dtype, None, rows=n, width=p)
    assert L.agp_kernelmatrix(ctx, DT[dtype], C.byref(kd), x.ptr, n, D, None, y.ptr, p, D, D, again.ptr, p) == 0
    assert _same(again, good) and _finite(again)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_linalg_blocks_refuse_small_leading_dimensions(env, dtype):
    """agp_potrf_jitter (lda), agp_spd_inverse (lda, ldi), agp_solve_right_spd (lda, ldb, ldx): ld = n - 1 is AGP_ERR_INVALID and nothing is
    written; the context solves correctly afterwards."""
    L, ctx = env["L"], env["ctx"]
    n, r = 100, 37
    rng, A = _spd(n, dtype)
    Bm = rng.standard_normal((r, n)).astype(NPT[dtype])
    a, b = _mk(dtype, None, data=A), _mk(dtype, None, data=Bm)
    a0 = a.bits()
    info = C.c_int32(-7)
    good = _mk(dtype, None, rows=r, width=n)
    assert L.agp_solve_right_spd(ctx, DT[dtype], a.ptr, n, n, b.ptr, n, r, good.ptr, n, C.byref(info)) == 0
    for name, lda, ldb, ldx in [("lda", n - 1, n, n), ("ldb", n, n - 1, n), ("ldx", n, n, n - 1)]:
        x = _mk(dtype, None, rows=r, width=n)
        st = L.agp_solve_right_spd(ctx, DT[dtype], a.ptr, lda, n, b.ptr, ldb, r, x.ptr, ldx, C.byref(info))
        assert L.agp_ctx_sync(ctx) == 0
        assert st == INVALID, ("agp_solve_right_spd", name, st)
        assert x.unwritten().all() and x.check(), name
    for name, lda, ldi in [("lda", n - 1, n), ("ldi", n, n - 1)]:
        inv = _mk(dtype, None, rows=n, width=n)
        st = L.agp_spd_inverse(ctx, DT[dtype], a.ptr, lda, n, inv.ptr, ldi, None, C.byref(info))
        assert st == INVALID, ("agp_spd_inverse", name, st)
        assert inv.unwritten().all() and inv.check(), name
    assert L.agp_potrf_jitter(ctx, DT[dtype], a.ptr, n - 1, n, 1e-4, C.byref(info)) == INVALID
    assert L.agp_ctx_sync(ctx) == 0
    assert np.array_equal(a.bits(), a0) and a.check() and b.check()
    again = _mk(dtype, None, rows=r, width=n)
    assert L.agp_solve_right_spd(ctx, DT[dtype], a.ptr, n, n, b.ptr, n, r, again.ptr, n, C.byref(info)) == 0
    assert _same(again, good) and info.value == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kmeans_refuses_small_leading_dimensions(env, dtype):
    L, ctx = env["L"], env["ctx"]
    rng = np.random.default_rng(4)
    n, D, m = 300, 16, 65
    X = rng.random((n, D))
    x, c = _mk(dtype, None, data=X), _mk(dtype, None, data=X[:m])
    c0 = c.bits()
    it, conv, obj = C.c_int32(), C.c_int32(), C.c_double()
    for ldx, ldc in [(D - 1, D), (D, D - 1)]:
        lab, md, cnt = _vec("i32", n), _vec(dtype, n), _vec("i32", m)
        assert L.agp_nearest_center(ctx, DT[dtype], x.ptr, n, ldx, D, c.ptr, ldc, m, lab.ptr, md.ptr) == INVALID
        assert L.agp_kmeans(ctx, DT[dtype], x.ptr, n, ldx, D, c.ptr, ldc, m, 10, 1e-3, lab.ptr, cnt.ptr, C.byref(it), C.byref(obj),
                            C.byref(conv)) == INVALID
        assert L.agp_ctx_sync(ctx) == 0
        assert all(q.unwritten().all() and q.check() for q in (lab, md, cnt)) and np.array_equal(c.bits(), c0) and c.check()
    lab, md = _vec("i32", n), _vec(dtype, n)
    assert L.agp_nearest_center(ctx, DT[dtype], x.ptr, n, D, D, c.ptr, D, m, lab.ptr, md.ptr) == 0
    assert L.agp_ctx_sync(ctx) == 0
    assert _written(lab, md) and np.array_equal(lab.window()[0, :m], np.arange(m))


def test_training_entry_points_refuse_small_ldx(env):
    """cavi_step, step_local, prefetch, elbo, elbo_enqueue with ldx = D - 1: AGP_ERR_INVALID, the posterior does not move, and the
    handle steps afterwards."""
    L = env["L"]
    rng = np.random.default_rng(7)
    N, D, m, B = 300, 3, 20, 64
    X, f, Z = _toy(rng, N, D, m)
    y = np.where(f + 0.2 * rng.standard_normal(N) > 0, 1.0, -1.0)
    h = Handle(env, "f64", Z, B, LIK_LOGISTIC, 1)
    x, yv = _mk("f64", None, data=X), _vec("f64", N, data=y)
    ix = _vec("i64", B, data=rng.choice(N, B, replace=False).astype(np.int64))
    h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, D, yv.ptr, ix.ptr, B, N / B))
    s0 = h.state()
    e, tk = C.c_double(), C.c_int32()
    assert L.agp_svgp_cavi_step(h.h, x.ptr, D - 1, yv.ptr, ix.ptr, B, N / B) == INVALID
    assert L.agp_svgp_step_local(h.h, x.ptr, D - 1, yv.ptr, ix.ptr, B, N / B) == INVALID
    assert L.agp_svgp_prefetch(h.h, x.ptr, D - 1, ix.ptr, B) == INVALID
    assert L.agp_svgp_elbo(h.h, x.ptr, D - 1, yv.ptr, ix.ptr, B, N / B, 1, C.byref(e)) == INVALID
    assert L.agp_svgp_elbo_enqueue(h.h, x.ptr, D - 1, yv.ptr, ix.ptr, B, N / B, 1, C.byref(tk)) == INVALID
    for a, b in zip(s0, h.state()):
        assert _same(a, b)
    h.ok(L.agp_svgp_cavi_step(h.h, x.ptr, D, yv.ptr, ix.ptr, B, N / B))
    h.ok(L.agp_svgp_check_status(h.h))
    s1 = h.state()
    assert _finite(*s1) and not _same(s1[2], s0[2])
    _checks(x, yv, ix)
    h.close()
