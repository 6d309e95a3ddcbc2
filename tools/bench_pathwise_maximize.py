#!/usr/bin/env python
"""Multi-start ascent of pathwise samples: the time of one agp_pathwise_maximize call next to what a caller can build from
paths.grad, one JSON line.

    python tools/bench_pathwise_maximize.py [--m 1024] [--features 1024] [--D 32] [--S 64] [--R 64] [--T 100] [--reps 10] [--warmup 2]

The model and the draw are those of tools/bench_pathwise.py.  (a) is the new call, S R particles for T steps in one launch.  (b) is
the loop of a caller without it: T times paths.grad on the S R device points (every path at every point), the gather of each
particle's own path, and the same ADAM update and clip in torch on the device.  Both are bracketed by device events after a warm-up;
reported are the medians over `reps` runs (and the minima), their ratio, and the largest difference of the two results.  A run
without a GPU fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def medians(torch, reps, warmup, call):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--features", type=int, default=1024)
    p.add_argument("--D", type=int, default=32)
    p.add_argument("--S", type=int, default=64)
    p.add_argument("--R", type=int, default=64)
    p.add_argument("--T", type=int, default=100)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--skip-loop", action="store_true", help="time the new call only")
    a = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pathwise_maximize.py needs a GPU: there is no CPU fallback")
    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    rng = np.random.default_rng(0)
    N, B = 20000, 1024
    X = rng.random((N, a.D))
    y = np.sign(np.sin(3 * X[:, 0]) + X[:, 1 % a.D] - 0.8 + 0.2 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:a.m]].copy()
    model = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                     optimiser=False, seed=0)
    AGP.train_(model, X, y, 3)
    dev = model._dev()
    S, R, D, T = a.S, a.R, a.D, a.T
    paths = AGP.sample_paths(model, S, n_features=a.features, seed=1, t=S)
    X0 = torch.rand(S, R, D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    lo, hi, lr = np.zeros(D), np.ones(D), np.full(D, 0.02)
    b1, b2, eps = 0.9, 0.999, 1e-8
    Xo = torch.empty(S, R, D, dtype=torch.float64, device=dev)
    Fo = torch.empty(S, R, dtype=torch.float64, device=dev)
    as_p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(T, 0, 0, b1, b2, eps, as_p(lo), as_p(hi), as_p(lr))

    def new_call():
        st = L.agp_pathwise_maximize(paths._p, 0, C.c_void_p(X0.data_ptr()), D, R, C.byref(opts), C.c_void_p(Xo.data_ptr()), D,
                                     C.c_void_p(Fo.data_ptr()), R, None, 0, None, None)
        if st != 0:
            raise RuntimeError(L.agp_last_error(model._ctx).decode())

    own = torch.arange(S, device=dev).repeat_interleave(R)
    pts = torch.arange(S * R, device=dev)
    tlo, thi, tlr = (torch.as_tensor(v, device=dev) for v in (lo, hi, lr))
    loop_out = {}

    def callers_loop():
        x = torch.minimum(torch.maximum(X0.reshape(S * R, D), tlo), thi)
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        b1k = b2k = 1.0
        for _ in range(T):
            g = paths.grad(x)[own, pts]  # (S, S R, D) from the device, of which each particle reads its own path's row
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            b1k, b2k = b1k * b1, b2k * b2
            x = torch.minimum(torch.maximum(x + tlr * ((m / (1 - b1k)) / (torch.sqrt(v / (1 - b2k)) + eps)), tlo), thi)
        loop_out["x"] = x

    na = medians(torch, a.reps, a.warmup, new_call)
    out = {"metric": "pathwise_maximize_ms", "m": a.m, "n_features": a.features, "D": D, "S": S, "R": R, "T": T, "reps": a.reps,
           "timing": "device events around each run, median (min), fp64", "maximize_ms": round(na[0], 3),
           "maximize_min_ms": round(na[1], 3)}
    if not a.skip_loop:
        lb = medians(torch, a.reps, a.warmup, callers_loop)
        diff = float((loop_out["x"].reshape(S, R, D) - Xo).abs().max())
        out.update({"grad_loop_ms": round(lb[0], 3), "grad_loop_min_ms": round(lb[1], 3), "loop_over_maximize": round(lb[0] / na[0], 2),
                    "max_abs_difference_of_x": diff})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
