"""Times the matrix-free kernel operator (agp_kernel_matmul, csrc/agp_kmv.h): out = K(X, X) V, fp64, HIP events around the call (which
prepares the Y side, launches and synchronises), against the only alternative there was before it: agp_kernelmatrix into memory
(8 n p bytes) followed by a dense GEMM (torch.mm, i.e. the vendor BLAS: the C ABI has no stand-alone GEMM entry point).

    python tools/bench_kmv.py [--n 32768] [--D 32] [--r 1 32] [--reps 5] [--no-dense] [--big 100000] [--dtype f64 f32]

--big: the same product at a size whose kernel matrix (80 GB at 1e5) is not formed at all; 0 skips it.
Every row also times the derivative bilinear form on the same shape (agp_kernel_bilinear_grad, csrc/agp_kmv_grad.h: about
(3 DP + R) / (DP + R) times the MFMA work of the product) and reports the ratio of the two best times; --lml N adds the time of one
IterativeGP.log_marginal_likelihood(grad=True) at N points with its default 32 probes (0 skips it).
--dtype: which instances of the operator are timed (default both).  f32 adds, per row, `fused_f32` (agp_kernel_matmul with AGP_F32:
float arrays, csrc/agp_kmv_f32.h) and, as what one CG iteration pays, `apply_f64` / `apply_f32`: agp_gp_cg_apply of a solver handle
(no preconditioner; Float64 V and Out, the sides prepared once at create) on the Float64 and on the Float32 operator, with the
ratios of the best times; --lml then times the log marginal likelihood on each operator (tol 1e-4) and reports the CG iterations.
--dx NT: the derivative with respect to the row points (agp_kernel_matmul_dx, csrc/agp_kmv_dx.h) for NT row points against p = --n
and p = --big column points, per r, beside agp_kernel_matmul's cross product on the same shapes, with the ratio of the best times and
the ratio of the MFMA counts (1 + CB) DP ceil(r / CB) / (DP + R); --predgrad N: one predict_f_grad(cov=True) of an IterativeGP on 32
test points at N training points, split into the batched solve and the gradient kernel's two launches (0 skips either).
--wide: the block of 128 columns (agp_kernel_matmul_wide, csrc/agp_kmv_wide.h; IterativeGP(block=128)) against the block of 32 on the
same build and nothing else: one product at n = p = --n with r = 128 (one wide launch against four launches of 32), one CG iteration at
N = --big at both blocks, and predict_f's variance for 128 test points at N = --big at both blocks (see wide_block).
--hd: the operator for 65 .. 128 input dimensions (agp_kernel_matmul_hd, csrc/agp_kmv_hd.h; see high_dim): one product of 32 columns
on prepared operators at D = 96 and 128 beside k_kmv at D = 64 and the dense composition, one CG iteration and one predictive
variance of 32 points at N = --big, D = 96.
--paths NT: one evaluation of 32 pathwise draws of an IterativeGP (agp_gp_cg_pathwise_eval, csrc/agp_path.h) at NT points against
N = --n training points and --features random features, (a) `fused`; (b) `composed`, the same result from what there was before:
agp_pathwise_eval of a 64-point GP's draw with the same number of features (k_pw_features into memory, 64 columns of kernel matrix,
one GEMM) plus agp_kernel_matmul's cross product against the N points; (c) `matmul_same_columns`, agp_kernel_matmul alone at
p = N + features columns: what the fused walk should approach; and `paths_eval_f32`, the Float32 instance (agp_gp_cg_pathwise_eval_f32,
csrc/agp_path_f32.h) against the Float64 one on the same paths object, alternating inside every repetition, the first Float32 call
(which prepares the Float32 side) timed on its own.  --paths-draw N adds one whole draw (tables, Phi(X) W, the batched CG
at tol 1e-6 with the default preconditioner) of 32 paths at N points.
Prints one JSON line; kernel values per second count n * p evaluations.  A record, not a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as g


def timed(fn, reps):
    ms = []
    for rep in range(reps + 1):  # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(best_ms=round(ms[0], 3), median_ms=round(ms[len(ms) // 2], 3))


def wide_block(a, AGP, capi, L, ctx, kd, gen):
    """--wide: the block of 128 (csrc/agp_kmv_wide.h) against the block of 32 on the same build, the two alternating inside every
    repetition.  (1) one product at n = p = --n, r = 128: one launch of agp_kernel_matmul_wide against four of agp_kernel_matmul,
    and the two results compared bit for bit -- whole calls, each with its own preparation of Y, workspace and synchronise -- and the
    same product by agp_gp_cg_apply on two prepared handles (`product_prepared`), which pays none of that; (2) one CG iteration at N = --big with the default preconditioner, r = block columns
    that never converge (tol = 0): the difference of a solve of 5 and a solve of 1 iterations, over 4; (3) predict_f's variance for
    128 test points at N = --big (alpha solved before the clock starts), host clock around a call that ends synchronised.  (1) is the
    best and median of --reps alternating repetitions; (2) the smaller of two runs per length; (3) ONE run per block."""
    import time

    import numpy as np

    res = dict(bench="kernel_matmul_wide", D=a.D)
    n, r = a.n, 128
    X = torch.rand(n, a.D, dtype=torch.float64, device="cuda", generator=gen)
    V = torch.randn(n, r, dtype=torch.float64, device="cuda", generator=gen)
    ow, o4 = torch.empty(n, r, dtype=torch.float64, device="cuda"), torch.empty(n, r, dtype=torch.float64, device="cuda")

    def product(call, c0, w, out):
        st = call(ctx, capi.F64, C.byref(kd), X.data_ptr(), n, a.D, None, n, 0, a.D, 1, 0.0, V.data_ptr() + 8 * c0, r, w, 0,
                  out.data_ptr() + 8 * c0, r)
        assert st == 0, L.agp_last_error(ctx)

    def four():
        for c0 in range(0, r, 32):
            product(L.agp_kernel_matmul, c0, 32, o4)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    wide = lambda: product(L.agp_kernel_matmul_wide, 0, r, ow)  # noqa: E731
    tw, t4 = [], []
    for rep in range(a.reps + 1):  # (repetition 0: the warm-up of both)
        tw.append(once(wide))
        t4.append(once(four))
    tw, t4 = sorted(tw[1:]), sorted(t4[1:])
    res["product"] = dict(n=n, r=r, wide_ms=dict(best=round(tw[0], 3), median=round(tw[len(tw) // 2], 3)),
                          four_launches_ms=dict(best=round(t4[0], 3), median=round(t4[len(t4) // 2], 3)),
                          wide_over_four=round(tw[0] / t4[0], 3),
                          bitwise_equal=bool(torch.equal(ow.view(torch.int64), o4.view(torch.int64))))
    # the same product on prepared operators (agp_gp_cg_apply, no preconditioner): no preparation of Y, no allocation per call
    hs = {}
    for b in (32, 128):
        hs[b] = C.c_void_p()
        assert L.agp_gp_cg_create(ctx, C.byref(kd), X.data_ptr(), n, a.D, a.D, 1e-2, 0, C.byref(hs[b]), None) == 0
        assert L.agp_gp_cg_set_block(hs[b], b) == 0

    def apply(b, out):
        for c0 in range(0, r, b):
            assert L.agp_gp_cg_apply(hs[b], V.data_ptr() + 8 * c0, r, b, out.data_ptr() + 8 * c0, r) == 0

    tw, t4 = [], []
    for rep in range(a.reps + 1):
        tw.append(once(lambda: apply(128, ow)))
        t4.append(once(lambda: apply(32, o4)))
    tw, t4 = sorted(tw[1:]), sorted(t4[1:])
    res["product_prepared"] = dict(n=n, r=r, wide_ms=dict(best=round(tw[0], 3), median=round(tw[len(tw) // 2], 3)),
                                   four_launches_ms=dict(best=round(t4[0], 3), median=round(t4[len(t4) // 2], 3)),
                                   wide_over_four=round(tw[0] / t4[0], 3),
                                   bitwise_equal=bool(torch.equal(ow.view(torch.int64), o4.view(torch.int64))))
    for h in hs.values():
        L.agp_gp_cg_destroy(h)
    del X, V, ow, o4
    N = a.big
    Xb = torch.rand(N, a.D, dtype=torch.float64, device="cuda", generator=gen).cpu().numpy()
    y = np.sin(3 * Xb[:, 0])
    Xt = np.random.default_rng(0).random((128, a.D))
    its, var = {}, {}
    models = {b: AGP.IterativeGP(Xb, y, AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale), noise=1e-2, tol=1e-6, block=b)
              for b in (32, 128)}
    for b, m in models.items():
        m.alpha()
        B = torch.randn(N, b, dtype=torch.float64, device="cuda", generator=gen)
        m._solve_dev(B, 0.0, 1)  # warm-up
        ts = {k: min(once(lambda: m._solve_dev(B, 0.0, k)) for _ in range(2)) for k in (1, 5)}
        its[b] = dict(iteration_ms=round((ts[5] - ts[1]) / 4, 3), per_column_ms=round((ts[5] - ts[1]) / 4 / b, 4))
    for b, m in models.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = AGP.predict_f(m, Xt)[1]
        var[b] = dict(seconds=round(time.perf_counter() - t0, 3), iterations=int(m.info["iterations"].max()), values=v)
    res["cg_iteration"] = dict(N=N, **{f"block{b}": its[b] for b in its})
    res["predict_f_variance_128_points"] = dict(N=N, max_abs_diff=float(np.abs(var[32]["values"] - var[128]["values"]).max()),
                                                **{f"block{b}": {k: var[b][k] for k in ("seconds", "iterations")} for b in var})
    for m in models.values():
        m.close()
    return res


def high_dim(a, AGP, capi, L, ctx, gen):
    """--hd: the operator for 65 .. 128 input dimensions (csrc/agp_kmv_hd.h).  (1) one product at n = p = --n, r = 32 on PREPARED
    operators (agp_gp_cg_apply of handles without preconditioner) at D = 96 and D = 128, alternating in every repetition with
    k_kmv at D = 64 on the same shape -- the d2 step grows with the padded width, the function and product steps do not --, and the
    dense composition at the same n: agp_kernelmatrix into memory plus torch.mm.  (2) at N = --big, D = 96: one CG iteration with the
    default preconditioner (the difference of a solve of 5 and of 1 iterations at tol = 0, over 4) and predict_f's variance for 32
    test points (alpha solved before the clock starts; host clock, ONE run)."""
    import time

    import numpy as np

    n, r = a.n, 32
    kern = lambda D: AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale * (32.0 / D) ** 0.5)  # noqa: E731
    V = torch.randn(n, r, dtype=torch.float64, device="cuda", generator=gen)
    out = torch.empty(n, r, dtype=torch.float64, device="cuda")
    Xs, hs, keep = {}, {}, []
    for D in (64, 96, 128):
        Xs[D] = torch.rand(n, D, dtype=torch.float64, device="cuda", generator=gen)
        kd, k = kern(D).desc(D)
        keep.append(k)
        hs[D] = C.c_void_p()
        assert L.agp_gp_cg_create(ctx, C.byref(kd), Xs[D].data_ptr(), n, D, D, 1e-2, 0, C.byref(hs[D]), None) == 0, L.agp_last_error(ctx)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ts = {D: [] for D in hs}
    for rep in range(a.reps + 1):  # (repetition 0: the warm-up of all three)
        for D, h in hs.items():
            ts[D].append(once(lambda: L.agp_gp_cg_apply(h, V.data_ptr(), r, r, out.data_ptr(), r)))
    res = dict(bench="kernel_matmul_hd", n=n, r=r, product_prepared={})
    for D in hs:
        t = sorted(ts[D][1:])
        res["product_prepared"][f"D{D}"] = dict(best_ms=round(t[0], 3), median_ms=round(t[len(t) // 2], 3),
                                                over_D64=round(t[0] / sorted(ts[64][1:])[0], 3))
        L.agp_gp_cg_destroy(hs[D])
    if not a.no_dense:
        K = torch.empty(n, n, dtype=torch.float64, device="cuda")
        for D in (96, 128):
            kd, k = kern(D).desc(D)

            def two_step():
                assert L.agp_kernelmatrix(ctx, capi.F64, C.byref(kd), Xs[D].data_ptr(), n, D, None, Xs[D].data_ptr(), n, D, D,
                                          K.data_ptr(), n) == 0, L.agp_last_error(ctx)
                return torch.mm(K, V)

            res["product_prepared"][f"D{D}"]["kernelmatrix_then_gemm"] = timed(two_step, a.reps)
        del K
    del Xs, V, out
    if a.big:
        N, D = a.big, 96
        Xb = torch.rand(N, D, dtype=torch.float64, device="cuda", generator=gen).cpu().numpy()
        m = AGP.IterativeGP(Xb, np.sin(3 * Xb[:, 0]), kern(D), noise=1e-2, tol=1e-6)
        m.alpha()
        B = torch.randn(N, r, dtype=torch.float64, device="cuda", generator=gen)
        m._solve_dev(B, 0.0, 1)  # warm-up
        tk = {k: min(once(lambda: m._solve_dev(B, 0.0, k)) for _ in range(2)) for k in (1, 5)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        AGP.predict_f(m, Xb[:32] + 0.01)
        res["big"] = dict(N=N, D=D, cg_iteration_ms=round((tk[5] - tk[1]) / 4, 3), alpha_iterations=int(m.alpha_info["iterations"].max()),
                          predict_f_variance_32_points=dict(seconds=round(time.perf_counter() - t0, 3),
                                                            iterations=int(m.info["iterations"].max())))
        m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--r", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--lml", type=int, default=0)
    ap.add_argument("--dx", type=int, default=0)
    ap.add_argument("--predgrad", type=int, default=0)
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--paths-draw", type=int, default=0)
    ap.add_argument("--dtype", nargs="+", choices=["f64", "f32"], default=["f64", "f32"])
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--hd", action="store_true")
    a = ap.parse_args()
    g.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    kd, keep = (AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale)).desc(a.D)
    gen = torch.Generator("cuda").manual_seed(0)
    res = dict(bench="kernel_matmul", D=a.D, sizes=[])

    def fused(X, V, out):
        n, r = X.shape[0], V.shape[1]
        st = L.agp_kernel_matmul(ctx, capi.F64, C.byref(kd), X.data_ptr(), n, a.D, None, n, 0, a.D, 1, 0.0, V.data_ptr(), r, r, 0,
                                 out.data_ptr(), r)
        assert st == 0, L.agp_last_error(ctx)

    if a.wide:
        print(json.dumps(wide_block(a, AGP, capi, L, ctx, kd, gen)))
        return
    if a.hd:
        print(json.dumps(high_dim(a, AGP, capi, L, ctx, gen)))
        return

    for n in [a.n] + ([a.big] if a.big else []):
        X = torch.rand(n, a.D, dtype=torch.float64, device="cuda", generator=gen)
        dense = not a.no_dense and n == a.n
        K = torch.empty(n, n, dtype=torch.float64, device="cuda") if dense else None
        for r in a.r:
            V = torch.randn(n, r, dtype=torch.float64, device="cuda", generator=gen)
            out = torch.empty(n, r, dtype=torch.float64, device="cuda")
            row = dict(n=n, r=r, fused=timed(lambda: fused(X, V, out), a.reps))
            row["fused_gvalues_per_s"] = round(n * n / row["fused"]["best_ms"] / 1e6, 1)
            if "f32" in a.dtype:
                Xf, Vf, outf = X.float(), V.float(), torch.empty(n, r, dtype=torch.float32, device="cuda")

                def fused32():
                    st = L.agp_kernel_matmul(ctx, capi.F32, C.byref(kd), Xf.data_ptr(), n, a.D, None, n, 0, a.D, 1, 0.0, Vf.data_ptr(), r,
                                             r, 0, outf.data_ptr(), r)
                    assert st == 0, L.agp_last_error(ctx)

                row["fused_f32"] = timed(fused32, a.reps)
                row["max_abs_diff_f32_vs_f64"] = float((outf.double() - out).abs().max())
                h = C.c_void_p()
                assert L.agp_gp_cg_create(ctx, C.byref(kd), X.data_ptr(), n, a.D, a.D, 1e-2, 0, C.byref(h), None) == 0
                for name, dt in (("apply_f64", capi.F64), ("apply_f32", capi.F32)):
                    assert L.agp_gp_cg_set_operator_dtype(h, dt) == 0
                    row[name] = timed(lambda: L.agp_gp_cg_apply(h, V.data_ptr(), r, r, out.data_ptr(), r), a.reps)
                L.agp_gp_cg_destroy(h)
                row["f64_over_f32"] = dict(abi=round(row["fused"]["best_ms"] / row["fused_f32"]["best_ms"], 3),
                                           apply=round(row["apply_f64"]["best_ms"] / row["apply_f32"]["best_ms"], 3))
                fused(X, V, out)  # (out again the Float64 product, for max_abs_diff below)
            U, dv, ds = torch.randn(n, r, dtype=torch.float64, device="cuda", generator=gen), C.c_double(), (C.c_double * a.D)()

            def grad():
                st = L.agp_kernel_bilinear_grad(ctx, capi.F64, C.byref(kd), X.data_ptr(), n, a.D, a.D, U.data_ptr(), r, V.data_ptr(),
                                                r, r, None, 0, C.byref(dv), ds)
                assert st == 0, L.agp_last_error(ctx)

            row["bilinear_grad"] = timed(grad, a.reps)
            row["grad_over_fused"] = round(row["bilinear_grad"]["best_ms"] / row["fused"]["best_ms"], 3)
            if dense:
                def two_step():
                    st = L.agp_kernelmatrix(ctx, capi.F64, C.byref(kd), X.data_ptr(), n, a.D, None, X.data_ptr(), n, a.D, a.D,
                                            K.data_ptr(), n)
                    assert st == 0, L.agp_last_error(ctx)
                    return torch.mm(K, V)

                row["kernelmatrix_then_gemm"] = timed(two_step, a.reps)
                ref = two_step()
                row["max_abs_diff"] = float((ref - out).abs().max())
            res["sizes"].append(row)
        del X, K
    if a.dx:
        res["matmul_dx"] = []
        DP = 16 if a.D <= 16 else 32 if a.D <= 32 else 64
        Xr = torch.rand(a.dx, a.D, dtype=torch.float64, device="cuda", generator=gen)
        for p in [a.n] + ([a.big] if a.big else []):
            Y = torch.rand(p, a.D, dtype=torch.float64, device="cuda", generator=gen)
            for r in a.r:
                V = torch.randn(p, r, dtype=torch.float64, device="cuda", generator=gen)
                o1, oD = torch.empty(a.dx, r, dtype=torch.float64, device="cuda"), torch.empty(a.dx, r * a.D, dtype=torch.float64, device="cuda")

                def cross():
                    st = L.agp_kernel_matmul(ctx, capi.F64, C.byref(kd), Xr.data_ptr(), a.dx, a.D, Y.data_ptr(), p, a.D, a.D, 0, 0.0,
                                             V.data_ptr(), r, r, 0, o1.data_ptr(), r)
                    assert st == 0, L.agp_last_error(ctx)

                def dx():
                    st = L.agp_kernel_matmul_dx(ctx, capi.F64, C.byref(kd), Xr.data_ptr(), a.dx, a.D, Y.data_ptr(), p, a.D, a.D,
                                                V.data_ptr(), r, r, 0, 0, oD.data_ptr(), r * a.D)
                    assert st == 0, L.agp_last_error(ctx)

                cb = 1 if r == 1 else 4
                row = dict(n=a.dx, p=p, r=r, CB=cb, matmul_dx=timed(dx, a.reps), matmul=timed(cross, a.reps))
                row["dx_over_matmul"] = round(row["matmul_dx"]["best_ms"] / row["matmul"]["best_ms"], 3)
                row["mfma_ratio"] = round((1 + cb) * DP * -(-r // cb) / (DP + 16 * -(-r // 16)), 3)
                res["matmul_dx"].append(row)
    if a.predgrad:
        from agp_amd import iterative

        Xh = torch.rand(a.predgrad, a.D, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).numpy()
        m = AGP.IterativeGP(Xh, Xh[:, 0].copy(), AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale), noise=1e-2, tol=1e-6)
        m.alpha()
        Xt = m._cx.dev_tensor(Xh[:32] + 0.01)
        sol, od = iterative._kstar_solve(m, Xt)[1], torch.empty(32, a.D, dtype=torch.float64, device="cuda")

        def kernels():
            for v, prd in ((m._alpha, 0), (sol, 1)):
                assert L.agp_gp_cg_apply_dx(m._h, Xt.data_ptr(), 32, a.D, v.data_ptr(), v.stride(0), v.shape[1], prd, od.data_ptr(),
                                            a.D) == 0

        res["predict_f_grad"] = dict(N=a.predgrad, nt=32, total=timed(lambda: AGP.predict_f_grad(m, Xh[:32] + 0.01), 1),
                                     solve=timed(lambda: iterative._kstar_solve(m, Xt), 1),
                                     gradient_kernels=timed(kernels, a.reps), iterations=int(m.info["iterations"].max()),
                                     converged=bool(m.info["converged"].all()))
        m.close()
    if a.paths or a.paths_draw:
        import numpy as np

        kern, S = AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale), 32
        hgen = torch.Generator().manual_seed(3)

        def model(n):
            Xh = torch.rand(n, a.D, dtype=torch.float64, generator=hgen).numpy()
            return AGP.IterativeGP(Xh, np.sin(Xh.sum(axis=1)), kern, noise=1e-2, tol=1e-6)

        if a.paths:
            nt, m = a.paths, model(a.n)
            paths = AGP.sample_paths(m, S, n_features=a.features, seed=1)
            Xt = torch.rand(nt, a.D, dtype=torch.float64, device="cuda", generator=gen)
            of, oc, ok = (torch.empty(nt, S, dtype=torch.float64, device="cuda") for _ in range(3))
            gp = AGP.GP(m.X[:64], m.y[:64], kern, noise=1e-2, optimiser=False, opt_noise=False)
            AGP.train_(gp, 1)
            small = AGP.sample_paths(gp, S, n_features=a.features, seed=1)
            Fs = torch.empty(S, nt, dtype=torch.float64, device="cuda")
            V = torch.randn(a.n, S, dtype=torch.float64, device="cuda", generator=gen)
            Vb = torch.randn(a.n + a.features, S, dtype=torch.float64, device="cuda", generator=gen)
            Yb = torch.rand(a.n + a.features, a.D, dtype=torch.float64, device="cuda", generator=gen)

            def cross(Y, Vm, out):
                st = L.agp_kernel_matmul(ctx, capi.F64, C.byref(kd), Xt.data_ptr(), nt, a.D, Y.data_ptr(), Y.shape[0], a.D, a.D, 0, 0.0,
                                         Vm.data_ptr(), S, S, 0, out.data_ptr(), S)
                assert st == 0, L.agp_last_error(ctx)

            def fused_eval():
                assert L.agp_gp_cg_pathwise_eval(paths._p, Xt.data_ptr(), a.D, nt, 0, of.data_ptr(), S) == 0
                assert L.agp_ctx_sync(m._cx.ctx) == 0

            def composed():
                assert L.agp_pathwise_eval(small._p, Xt.data_ptr(), a.D, nt, Fs.data_ptr(), nt) == 0
                assert L.agp_ctx_sync(gp._ctx) == 0
                cross(m._Xd, V, oc)

            res["paths_eval"] = dict(N=a.n, L=a.features, nt=nt, S=S, fused=timed(fused_eval, a.reps), composed=timed(composed, a.reps),
                                     matmul_same_columns=timed(lambda: cross(Yb, Vb, ok), a.reps))
            # the Float32 instance (csrc/agp_path_f32.h) against the Float64 one, alternating inside every repetition; the first
            # Float32 call, which prepares the Float32 side of the snapshot, is timed on its own
            o32 = torch.empty(nt, S, dtype=torch.float32, device="cuda")

            def fused_eval32():
                assert L.agp_gp_cg_pathwise_eval_f32(paths._p, Xt.data_ptr(), a.D, nt, 0, o32.data_ptr(), S) == 0
                assert L.agp_ctx_sync(m._cx.ctx) == 0

            def clock(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            first = clock(fused_eval32)
            t64, t32 = [], []
            for _ in range(max(a.reps, 5)):
                t64.append(clock(fused_eval))
                t32.append(clock(fused_eval32))
            t64.sort(), t32.sort()
            err = float(((o32.double() - of).abs().max() / of.abs().max()).item())
            res["paths_eval_f32"] = dict(N=a.n, L=a.features, nt=nt, S=S, D=a.D, first_call_ms=round(first, 3),
                                         f64=dict(best_ms=round(t64[0], 3), median_ms=round(t64[len(t64) // 2], 3), max_ms=round(t64[-1], 3)),
                                         f32=dict(best_ms=round(t32[0], 3), median_ms=round(t32[len(t32) // 2], 3), max_ms=round(t32[-1], 3)),
                                         ratio_median=round(t64[len(t64) // 2] / t32[len(t32) // 2], 3), max_diff_rel=err)
            paths.free()
            small.free()
            m.close()
        if a.paths_draw:
            m = model(a.paths_draw)
            m._solver()  # (the handle and its preconditioner are not part of the draw)
            box = []
            t = timed(lambda: box.append(AGP.sample_paths(m, S, n_features=a.features, seed=1, t=len(box))), 1)
            res["paths_draw"] = dict(N=a.paths_draw, L=a.features, S=S, **t, iterations=int(box[-1].info["iterations"].max()),
                                     converged=bool(box[-1].info["converged"].all()))
            for pth in box:
                pth.free()
            m.close()
    if a.lml:
        Xh = torch.rand(a.lml, a.D, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).numpy()
        import numpy as np

        for dt in a.dtype:
            m = AGP.IterativeGP(Xh, Xh[:, 0].copy(), AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale), noise=1e-2,
                                tol=1e-6 if a.dtype == ["f64"] else 1e-4, operator_dtype=np.float32 if dt == "f32" else np.float64)
            val = []
            t = timed(lambda: val.append(m.log_marginal_likelihood(grad=True)[0]), min(a.reps, 2))
            res["lml_grad" if dt == "f64" else "lml_grad_f32"] = dict(n=a.lml, **t, iterations=int(m.info["iterations"].max()),
                                                                       converged=bool(m.info["converged"].all()), value=val[-1])
            m.close()
    L.agp_ctx_destroy(ctx)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
