#!/usr/bin/env python
"""One agp_svgp_acq_maximize_batch call of q rounds against q separate agp_svgp_acq_maximize calls, on one GPU; one JSON line.

    python tools/bench_acq_batch.py [--m 1024] [--D 8] [--starts 4096] [--steps 100] [--q 8] [--warmup 2] [--reps 7]

The model, the data, the starts and the acquisition function (EI over the largest predicted mean at the starts, box [0, 1]^D, lr 0.02)
are those of tools/bench_acq.py.  In ONE process, alternating, every call between two device events:
  batch      one batch call: q rounds, round b on the predictor augmented by the b winners before (m' = m + b)
  separate   q calls of agp_svgp_acq_maximize on the same starts (each proposes the same point: the work a batch is compared with,
             not an alternative to it)
The separate calls run every step at m columns, the batch at m + b: the expectation from the code is a per-step factor of about
(m + b) / m, plus one bordering (four small launches and a rescale of Z') per round."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_acq import stats  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--D", type=int, default=8)
    p.add_argument("--starts", type=int, default=4096)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--q", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_acq_batch: no GPU visible (a timing needs the device)")
    L = capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    N, D, m, R, T, q = 20000, a.D, a.m, a.starts, a.steps, a.q
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X = torch.rand(N, D, dtype=torch.float64, device=dev, generator=g)
    y = torch.sin(3 * X[:, 0]) + X[:, min(1, D - 1)] - 0.8 + 0.1 * torch.randn(N, dtype=torch.float64, device=dev, generator=g)
    k = AGP.with_lengthscale(AGP.SqExponentialKernel(), math.sqrt(D) / 4.0)
    Z = X[torch.randperm(N, device=dev, generator=g)[:m]].cpu().numpy()
    model = AGP.SVGP(k, AGP.GaussianLikelihood(0.05), AGP.AnalyticSVI(m), Z, optimiser=False, seed=0)
    AGP.train_(model, X, y.cpu().numpy(), 10)
    X0 = torch.rand(R, D, dtype=torch.float64, device=dev, generator=g).contiguous()
    h = model._h
    ptr = lambda t: C.c_void_p(t.data_ptr())
    mu = torch.empty(R, dtype=torch.float64, device=dev)
    model._chk(L.agp_svgp_predict_f(h, ptr(X0), D, R, ptr(mu), None))
    lo, hi, lrv = np.zeros(D), np.ones(D), np.full(D, 0.02)
    as_p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(T, 0, 0, 0.9, 0.999, 1e-8, as_p(lo), as_p(hi), as_p(lrv))
    desc = capi.AcqDesc(capi.ACQ_EI, 0, 0.0, float(mu.max()), 0.01)
    xb, ab = torch.empty(q, D, dtype=torch.float64, device=dev), torch.empty(q, dtype=torch.float64, device=dev)
    ib = torch.empty(q, dtype=torch.int64, device=dev)
    x1, a1 = torch.empty(D, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)

    def batch():
        model._chk(L.agp_svgp_acq_maximize_batch(h, 0, C.byref(desc), None, D, 0, 0.0, q, ptr(X0), D, R, C.byref(opts), ptr(xb), D, ptr(ab),
                                                 ptr(ib)))

    def separate():
        for _ in range(q):
            model._chk(L.agp_svgp_acq_maximize(h, 0, C.byref(desc), ptr(X0), D, R, C.byref(opts), None, D, None, ptr(x1), ptr(a1), None))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = (batch, separate)
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[], []]
    for _ in range(a.reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    model._chk(L.agp_svgp_check_status(h))
    row = {"m": m, "D": D, "starts": R, "steps": T, "q": q, "acquisition": "EI", "batch": stats(ts[0]), "separate": stats(ts[1])}
    row["ratio_batch_over_separate"] = round(row["batch"]["median_ms"] / row["separate"]["median_ms"], 4)
    row["expected_from_columns"] = round(sum((m + b) / m for b in range(q)) / q, 4)
    row["first_point_same_bits"] = bool(torch.equal(xb[0], x1))
    row["distinct_points"] = int(torch.unique(xb, dim=0).shape[0])
    row["checksum"] = float(ab.sum())
    print(json.dumps({"metric": "acq_maximize_batch_ms", "warmup": a.warmup, "reps": a.reps,
                      "timing": "device events around each call; batch call and q separate calls alternating in one process",
                      "rows": [row]}))


if __name__ == "__main__":
    main()
