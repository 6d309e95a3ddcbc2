#!/usr/bin/env python
"""Streamed log predictive density (agp_svgp_lpd_stream) against its yardstick, agp_svgp_predict_f with variances over the same
points, on one GPU; one JSON line.

    python tools/bench_lpd.py [--shapes c2,c3] [--N 1000000] [--warmup 5] [--reps 20] [--nodes 100]

Shapes: c2 = SqExponential + Logistic, D = 32, m = 1024, fp64; c3 = Matern52 + StudentT(3), D = 64, m = 2048, fp32 (bench.py's C2 /
C3 models), N points U[0,1]^D, 10 AnalyticSVI(m) steps first so that the posterior is not the prior.  Per shape, in ONE process:
`warmup` evaluations of each, then `reps` rounds that ALTERNATE one lpd call and one predict_f(cov) over the same N points, every
call between two device events (the lpd call ends in its own synchronisation; predict_f is synchronised by the closing event).
Reported: median and the spread (min, max, inter-quartile range over the median) of both, and the ratio of the medians (the streamed
ELBO's ratio at c2 is 1.024).  The point-wise kernel's own time is not in here: take it from one
`rocprofv3 --kernel-trace --stats -- python tools/bench_lpd.py --shapes c2 --reps 3` run of its own (k_predict_lpd, k_lpd_reduce)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "c2": dict(kernel="sqexp", lik="logistic", m=1024, D=32, f32=False),
    "c3": dict(kernel="matern52", lik="studentt", m=2048, D=64, f32=True),
}


def stats(ms):
    a = np.sort(np.asarray(ms))
    med = float(np.median(a))
    q1, q3 = np.percentile(a, [25, 75])
    return {"median_ms": round(med, 3), "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3),
            "iqr_over_median": round(float((q3 - q1) / med), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="c2,c3")
    p.add_argument("--N", type=int, default=1_000_000)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--nodes", type=int, default=100)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_lpd: no GPU visible (a timing needs the device)")
    L = capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    x, w = AGP.gauss_hermite_rule(a.nodes)
    xp, wp = x.ctypes.data_as(C.POINTER(C.c_double)), w.ctypes.data_as(C.POINTER(C.c_double))
    rows = []
    for name in a.shapes.split(","):
        cfg = SHAPES[name]
        N, D, m = a.N, cfg["D"], cfg["m"]
        T = np.float32 if cfg["f32"] else np.float64
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        X64 = torch.rand(N, D, dtype=torch.float64, device=dev, generator=g)
        f = torch.sin(3 * X64[:, 0]) + X64[:, 1] - 0.8
        if cfg["lik"] == "logistic":
            lik, y = AGP.LogisticLikelihood(), torch.sign(f + 0.3 * torch.randn(N, dtype=torch.float64, device=dev, generator=g))
            y[y == 0] = 1.0
        else:
            lik, y = AGP.StudentTLikelihood(3.0, 1.0), f + 0.2 * torch.randn(N, dtype=torch.float64, device=dev, generator=g)
        base = AGP.SqExponentialKernel() if cfg["kernel"] == "sqexp" else AGP.Matern52Kernel()
        k = AGP.with_lengthscale(base, math.sqrt(D) / 4.0)
        Z = X64[torch.randperm(N, device=dev, generator=g)[:m]].cpu().numpy()
        model = AGP.SVGP(k, lik, AGP.AnalyticSVI(m), Z, optimiser=False, T=T)
        AGP.train_(model, X64, y.cpu().numpy(), 10)
        Xd = model._upload(X64)
        del X64
        yd = y.to(model.tdtype).contiguous()
        mu = torch.empty(N, dtype=model.tdtype, device=dev)
        var = torch.empty(N, dtype=model.tdtype, device=dev)
        out = C.c_double()

        def lpd():
            model._chk(L.agp_svgp_lpd_stream(model._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), N, xp, wp,
                                             len(x), C.byref(out), None))

        def predict():
            model._chk(L.agp_svgp_predict_f(model._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), N, C.c_void_p(mu.data_ptr()),
                                            C.c_void_p(var.data_ptr())))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            lpd()
            predict()
        torch.cuda.synchronize()
        tl, tp = [], []
        for _ in range(a.reps):
            tl.append(timed(lpd))
            tp.append(timed(predict))
        row = {"shape": name, "N": N, "D": D, "m": m, "dtype": "f32" if cfg["f32"] else "f64", "n_nodes": len(x), "lpd": out.value,
               "lpd_stream": stats(tl), "predict_f_var": stats(tp)}
        row["ratio_of_medians"] = round(row["lpd_stream"]["median_ms"] / row["predict_f_var"]["median_ms"], 4)
        rows.append(row)
        del model, Xd, yd, mu, var
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "lpd_stream_ms", "warmup": a.warmup, "reps": a.reps,
                      "timing": "device events around each call, streamed lpd and predict_f(cov) alternating in one process",
                      "rows": rows}))


if __name__ == "__main__":
    main()
