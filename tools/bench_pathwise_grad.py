#!/usr/bin/env python
"""Input gradients of pathwise samples: time of agp_pathwise_eval_grad next to agp_pathwise_eval on the same draw and points, one
JSON line.

    python tools/bench_pathwise_grad.py [--nt 100000] [--m 1024] [--features 1024] [--D 32] [--S 64] [--reps 10] [--warmup 2]

The model and the draw are those of tools/bench_pathwise.py.  Every call is bracketed by its own pair of device events after a
warm-up; reported are the medians over `reps` calls, and 2 D times the evaluation's median: what a central-difference gradient of
paths(X) would cost.  A run without a GPU fails.
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
    p.add_argument("--nt", type=int, default=100000)
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--features", type=int, default=1024)
    p.add_argument("--D", type=int, default=32)
    p.add_argument("--S", type=int, default=64)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pathwise_grad.py needs a GPU: there is no CPU fallback")
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
    Xt = torch.rand(a.nt, a.D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    paths = AGP.sample_paths(model, a.S, n_features=a.features, seed=1, t=a.S)
    F = torch.empty(a.S, a.nt, dtype=torch.float64, device=dev)
    Gr = torch.empty(a.S, a.nt, a.D, dtype=torch.float64, device=dev)
    px, pf, pg = (C.c_void_p(t.data_ptr()) for t in (Xt, F, Gr))

    def chk(st):
        if st != 0:
            raise RuntimeError(L.agp_last_error(model._ctx).decode())

    ev = medians(torch, a.reps, a.warmup, lambda: chk(L.agp_pathwise_eval(paths._p, px, a.D, a.nt, pf, a.nt)))
    gr = medians(torch, a.reps, a.warmup, lambda: chk(L.agp_pathwise_eval_grad(paths._p, px, a.D, a.nt, None, 0, pg, a.nt, a.D)))
    gv = medians(torch, a.reps, a.warmup, lambda: chk(L.agp_pathwise_eval_grad(paths._p, px, a.D, a.nt, pf, a.nt, pg, a.nt, a.D)))
    print(json.dumps({"metric": "pathwise_eval_grad_ms", "n_t": a.nt, "m": a.m, "n_features": a.features, "D": a.D, "S": a.S,
                      "reps": a.reps, "timing": "device events around each call, median (min), fp64",
                      "eval_ms": round(ev[0], 3), "eval_min_ms": round(ev[1], 3), "grad_ms": round(gr[0], 3),
                      "grad_min_ms": round(gr[1], 3), "grad_with_values_ms": round(gv[0], 3),
                      "central_difference_ms": round(2 * a.D * ev[0], 3), "fd_over_grad": round(2 * a.D * ev[0] / gr[0], 2)}))


if __name__ == "__main__":
    main()
