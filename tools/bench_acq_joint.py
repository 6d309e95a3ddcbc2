#!/usr/bin/env python
"""One agp_svgp_acq_maximize_joint call against agp_svgp_acq_maximize with as many particles, on one GPU; one JSON line.

    python tools/bench_acq_joint.py [--m 1024] [--D 8] [--q 8] [--starts 512] [--samples 256] [--steps 100] [--warmup 2] [--reps 7]
                                    [--only joint|single]

The model, the data, the box [0, 1]^D, lr 0.02 and the acquisition function (EI over the largest predicted mean at the starts) are
those of tools/bench_acq.py.  In ONE process, alternating, every call between two device events:
  joint    one joint call: `starts` q-tuples, q-EI over `samples` base samples (agp_mc_normals, seed 0)
  single   agp_svgp_acq_maximize on starts * q single points: the same number of particles, the same K*m and W work per step
Per step the joint call adds to the single one: the covariance kernel (q (q + 3) / 2 dot products over m per set), the per-set kernel
(Cholesky, S q^2 / 2 sample work, the backward pass), and the weight rows (2 q^2 m per set); the contraction and the two products in
front are the single call's.  The expectation from the code is a per-step ratio close to 1.  `--only` runs one side alone, for a
kernel trace."""
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
    p.add_argument("--q", type=int, default=8)
    p.add_argument("--starts", type=int, default=512)
    p.add_argument("--samples", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--only", choices=("joint", "single"), default=None)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_acq_joint: no GPU visible (a timing needs the device)")
    L = capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    N, D, m, R, T, q, S = 20000, a.D, a.m, a.starts, a.steps, a.q, a.samples
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X = torch.rand(N, D, dtype=torch.float64, device=dev, generator=g)
    y = torch.sin(3 * X[:, 0]) + X[:, min(1, D - 1)] - 0.8 + 0.1 * torch.randn(N, dtype=torch.float64, device=dev, generator=g)
    k = AGP.with_lengthscale(AGP.SqExponentialKernel(), math.sqrt(D) / 4.0)
    Z = X[torch.randperm(N, device=dev, generator=g)[:m]].cpu().numpy()
    model = AGP.SVGP(k, AGP.GaussianLikelihood(0.05), AGP.AnalyticSVI(m), Z, optimiser=False, seed=0)
    AGP.train_(model, X, y.cpu().numpy(), 10)
    X0 = torch.rand(R * q, D, dtype=torch.float64, device=dev, generator=g).contiguous()  # R tuples of q points = R q single starts
    h = model._h
    ptr = lambda t: C.c_void_p(t.data_ptr())
    mu = torch.empty(R * q, dtype=torch.float64, device=dev)
    model._chk(L.agp_svgp_predict_f(h, ptr(X0), D, R * q, ptr(mu), None))
    E = torch.empty(S, q, dtype=torch.float64, device=dev)
    model._chk(L.agp_mc_normals(model._ctx, 0, 0, 3, S, q, ptr(E)))
    lo, hi, lrv = np.zeros(D), np.ones(D), np.full(D, 0.02)
    as_p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(T, 0, 0, 0.9, 0.999, 1e-8, as_p(lo), as_p(hi), as_p(lrv))
    desc = capi.AcqDesc(capi.ACQ_EI, 0, 0.0, float(mu.max()), 0.01)
    xb, ab = torch.empty(q, D, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    x1, a1 = torch.empty(D, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)

    def joint():
        model._chk(L.agp_svgp_acq_maximize_joint(h, 0, C.byref(desc), None, D, 0, q, ptr(X0), D, R, ptr(E), q, S, C.byref(opts), None, D, None,
                                                 ptr(xb), D, ptr(ab), None))

    def single():
        model._chk(L.agp_svgp_acq_maximize(h, 0, C.byref(desc), ptr(X0), D, R * q, C.byref(opts), None, D, None, ptr(x1), ptr(a1), None))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = [f for f in (joint, single) if a.only in (None, f.__name__)]
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = {fn.__name__: [] for fn in fns}
    for _ in range(a.reps):
        for fn in fns:
            ts[fn.__name__].append(timed(fn))
    model._chk(L.agp_svgp_check_status(h))
    row = {"m": m, "D": D, "q": q, "starts": R, "samples": S, "steps": T, "particles": R * q, "acquisition": "EI"}
    for name, t in ts.items():
        row[name] = stats(t)
        row[name + "_ms_per_step"] = round(row[name]["median_ms"] / (T + 1), 5)
    if a.only is None:
        row["ratio_joint_over_single"] = round(row["joint"]["median_ms"] / row["single"]["median_ms"], 4)
    if "joint" in ts:
        row["checksum"] = float(ab[0])
    print(json.dumps({"metric": "acq_maximize_joint_ms", "warmup": a.warmup, "reps": a.reps,
                      "timing": "device events around each call; the joint call and the single-point call alternating in one process",
                      "rows": [row]}))


if __name__ == "__main__":
    main()
