#!/usr/bin/env python
"""Pathwise sampling: time of agp_pathwise_eval on one GPU next to predict_f over the same points, one JSON line.

    python tools/bench_pathwise.py [--nt 1000000] [--m 1024] [--features 1024] [--D 32] [--samples 1,64] [--reps 5] [--warmup 2]

An SVGP (Logistic, AnalyticSVI, m inducing points in D dimensions, a few steps) is drawn from with S samples and l features; the S
paths are then evaluated at n_t points.  Timed with device events around `reps` calls after a warm-up, per S: ms per
agp_pathwise_eval, the GEMM-shaped work 2 n_t (l + m) S over that time, and ms per agp_svgp_predict_f (means only, and with
variances) over the same points in the same run.  The time of the draw itself (host-synchronous: K refresh, one factorisation) is
reported from a host clock.  The share of the feature kernel is not visible to events around the whole call: take it from a kernel
trace of this script (k_pw_features against k_gemm_nt* and k_kernelmatrix_mma).  A run without a GPU fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, reps, warmup, call):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nt", type=int, default=1000000)
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--features", type=int, default=1024)
    p.add_argument("--D", type=int, default=32)
    p.add_argument("--samples", default="1,64")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pathwise.py needs a GPU: there is no CPU fallback")
    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    rng = np.random.default_rng(0)
    N, B = 20000, 1024
    X = rng.random((N, a.D))
    y = np.sign(np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 + 0.2 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:a.m]].copy()
    model = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                     optimiser=False, seed=0)
    AGP.train_(model, X, y, 3)
    dev = model._dev()
    Xt = torch.rand(a.nt, a.D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    px = C.c_void_p(Xt.data_ptr())

    def chk(st):
        if st != 0:
            raise RuntimeError(L.agp_last_error(model._ctx).decode())

    mu = torch.empty(1, a.nt, dtype=torch.float64, device=dev)
    var = torch.empty(1, a.nt, dtype=torch.float64, device=dev)
    pm, pv = C.c_void_p(mu.data_ptr()), C.c_void_p(var.data_ptr())
    rows = []
    predict = {
        "predict_f_mean_ms": round(timed(torch, a.reps, a.warmup, lambda: chk(L.agp_svgp_predict_f(model._h, px, a.D, a.nt, pm, None))), 3),
        "predict_f_var_ms": round(timed(torch, a.reps, a.warmup, lambda: chk(L.agp_svgp_predict_f(model._h, px, a.D, a.nt, pm, pv))), 3),
    }
    for S in [int(s) for s in a.samples.split(",")]:
        t0 = time.perf_counter()
        paths = AGP.sample_paths(model, S, n_features=a.features, seed=1, t=S)
        draw_ms = 1e3 * (time.perf_counter() - t0)
        out = torch.empty(S, a.nt, dtype=torch.float64, device=dev)
        po = C.c_void_p(out.data_ptr())
        ms = timed(torch, a.reps, a.warmup, lambda: chk(L.agp_pathwise_eval(paths._p, px, a.D, a.nt, po, a.nt)))
        gf = 2.0 * a.nt * (a.features + a.m) * S / 1e9
        # the mean over the samples against predict_f's mean: the draws are centred there given the features (a sanity figure)
        dmean = float((out.mean(dim=0) - mu[0]).abs().max()) if S > 1 else None
        rows.append({"S": S, "eval_ms": round(ms, 3), "gemm_gflop": round(gf, 1), "gemm_tflops": round(gf / ms, 3),
                     "draw_host_ms": round(draw_ms, 1), "max_abs_mean_minus_predict_f": dmean})
        paths.free()
        del out
    print(json.dumps({"metric": "pathwise_eval_ms", "n_t": a.nt, "m": a.m, "n_features": a.features, "D": a.D, "reps": a.reps,
                      "timing": "device events around the calls, fp64", **predict, "rows": rows}))


if __name__ == "__main__":
    main()
