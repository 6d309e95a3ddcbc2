#!/usr/bin/env python
"""Input gradients of the predictive moments (agp_svgp_predict_f_grad) against their floor, agp_svgp_predict_f with variances over the
same points (the gradient call contains that call's kernel matrix and a product of the same size), on one GPU; one JSON line.

    python tools/bench_predgrad.py [--N 1000000] [--m 1024] [--D 32] [--f32] [--warmup 3] [--reps 10]

SqExponential + Logistic, N points U[0,1]^D, 10 AnalyticSVI(m) steps first so that the posterior is not the prior (bench.py's C2
model at the defaults).  In ONE process: `warmup` evaluations of each, then `reps` rounds that ALTERNATE the gradient call with
variances, the means-only gradient call and predict_f(cov) over the same N points, every call between two device events.  Reported:
median and spread (min, max, inter-quartile range over the median) of the three, and the ratios of the medians to predict_f's.
The kernels' own times are not in here: take them from one `rocprofv3 --kernel-trace --stats -- python tools/bench_predgrad.py
--warmup 1 --reps 3` run of its own (k_predgrad against the k_gemm_nt* beside it)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.sort(np.asarray(ms))
    med = float(np.median(a))
    q1, q3 = np.percentile(a, [25, 75])
    return {"median_ms": round(med, 3), "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3),
            "iqr_over_median": round(float((q3 - q1) / med), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--N", type=int, default=1_000_000)
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--D", type=int, default=32)
    p.add_argument("--f32", action="store_true")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_predgrad: no GPU visible (a timing needs the device)")
    L = capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    N, D, m = a.N, a.D, a.m
    T = np.float32 if a.f32 else np.float64
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X64 = torch.rand(N, D, dtype=torch.float64, device=dev, generator=g)
    f = torch.sin(3 * X64[:, 0]) + X64[:, min(1, D - 1)] - 0.8
    y = torch.sign(f + 0.3 * torch.randn(N, dtype=torch.float64, device=dev, generator=g))
    y[y == 0] = 1.0
    k = AGP.with_lengthscale(AGP.SqExponentialKernel(), math.sqrt(D) / 4.0)
    Z = X64[torch.randperm(N, device=dev, generator=g)[:m]].cpu().numpy()
    model = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(m), Z, optimiser=False, T=T, seed=0)
    AGP.train_(model, X64, y.cpu().numpy(), 10)
    Xd = model._upload(X64)
    del X64
    mu = torch.empty(N, dtype=model.tdtype, device=dev)
    var = torch.empty(N, dtype=model.tdtype, device=dev)
    dmu = torch.empty(N, D, dtype=model.tdtype, device=dev)
    dvar = torch.empty(N, D, dtype=model.tdtype, device=dev)
    xp, ldx = C.c_void_p(Xd.data_ptr()), Xd.stride(0)

    def grad():
        model._chk(L.agp_svgp_predict_f_grad(model._h, xp, ldx, N, C.c_void_p(dmu.data_ptr()), C.c_void_p(dvar.data_ptr()), D))

    def grad_mean():
        model._chk(L.agp_svgp_predict_f_grad(model._h, xp, ldx, N, C.c_void_p(dmu.data_ptr()), None, D))

    def predict():
        model._chk(L.agp_svgp_predict_f(model._h, xp, ldx, N, C.c_void_p(mu.data_ptr()), C.c_void_p(var.data_ptr())))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = (grad, grad_mean, predict)
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[], [], []]
    for _ in range(a.reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    row = {"N": N, "D": D, "m": m, "dtype": "f32" if a.f32 else "f64", "predict_f_grad": stats(ts[0]),
           "predict_f_grad_means_only": stats(ts[1]), "predict_f_var": stats(ts[2]),
           "checksum": [float(dmu.double().abs().sum()), float(dvar.double().abs().sum())]}
    floor = row["predict_f_var"]["median_ms"]
    row["ratio_grad_over_predict_f"] = round(row["predict_f_grad"]["median_ms"] / floor, 4)
    row["ratio_means_only_over_predict_f"] = round(row["predict_f_grad_means_only"]["median_ms"] / floor, 4)
    print(json.dumps({"metric": "predict_f_grad_ms", "warmup": a.warmup, "reps": a.reps,
                      "timing": "device events around each call; gradient, means-only gradient and predict_f(cov) alternating in one process",
                      "rows": [row]}))


if __name__ == "__main__":
    main()
