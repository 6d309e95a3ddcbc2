#!/usr/bin/env python
"""The on-device acquisition maximiser (agp_svgp_acq_maximize) against the loop a user writes without it, on one GPU; one JSON line.

    python tools/bench_acq.py [--m 1024] [--D 32] [--starts 1024] [--steps 100] [--warmup 2] [--reps 7]
                                [--kind ei|pi|logei|logpi] [--incumbent-sds 0]

SqExponential + Gaussian SVGP, 20000 points U[0,1]^D, 10 AnalyticSVI(m) steps first so that the posterior is not the prior; expected
improvement over the largest predicted mean at the starts, box [0, 1]^D, lr 0.02.  In ONE process, alternating:
  device   one agp_svgp_acq_maximize call: `steps` ADAM steps of all starts, four launches per step, no host synchronisation
  host     the same ascent driven from the host on the same handle and the same starts: per step agp_svgp_predict_f (mean and variance)
           and agp_svgp_predict_f_grad on device tensors, then EI, the chain rule, the ADAM update and the clip in torch -- the
           moments never leave the device, which is the kindest form of that loop
every call between two device events.  Reported: the medians and spreads per call, per step, their ratio, the largest difference
of the two final alpha vectors (the loops are the same iteration), and for the device call the host's time to ENQUEUE a step (the
call returns before the device is done) next to the device's time per step: their quotient is the share of a step that the host
needs for its four launches -- at 1 the ascent is bound by launches, and a single-launch variant would have something to gain.
--kind picks the acquisition function of both loops (ei by default); --incumbent-sds puts the incumbent that many prior standard
deviations above the largest mean at the starts, which sends every start down the left tail (the log kinds' continued fraction)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

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
    p.add_argument("--m", type=int, default=1024)
    p.add_argument("--D", type=int, default=32)
    p.add_argument("--starts", type=int, default=1024)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--kind", choices=("ei", "pi", "logei", "logpi"), default="ei")
    p.add_argument("--incumbent-sds", type=float, default=0.0)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_acq: no GPU visible (a timing needs the device)")
    L = capi.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    N, D, m, R, T = 20000, a.D, a.m, a.starts, a.steps
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
    mu, var = (torch.empty(R, dtype=torch.float64, device=dev) for _ in range(2))
    dmu, dvar = (torch.empty(R, D, dtype=torch.float64, device=dev) for _ in range(2))
    model._chk(L.agp_svgp_predict_f(h, ptr(X0), D, R, ptr(mu), ptr(var)))
    best, xi, lr, b1, b2, eps = float(mu.max()) + a.incumbent_sds * math.sqrt(float(k.variance)), 0.01, 0.02, 0.9, 0.999, 1e-8
    lo, hi, lrv = np.zeros(D), np.ones(D), np.full(D, lr)
    as_p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    opts = capi.PwAscentOpts(T, 0, 0, b1, b2, eps, as_p(lo), as_p(hi), as_p(lrv))
    code = {"ei": capi.ACQ_EI, "pi": capi.ACQ_PI, "logei": capi.ACQ_LOG_EI, "logpi": capi.ACQ_LOG_PI}[a.kind]
    desc = capi.AcqDesc(code, 0, 0.0, best, xi)
    Xo, Ao = torch.empty(R, D, dtype=torch.float64, device=dev), torch.empty(R, dtype=torch.float64, device=dev)
    enqueue = []

    def device():
        t0 = time.perf_counter()
        model._chk(L.agp_svgp_acq_maximize(h, 0, C.byref(desc), ptr(X0), D, R, C.byref(opts), ptr(Xo), D, ptr(Ao), None, None, None))
        enqueue.append((time.perf_counter() - t0) * 1e3)

    def ei(x):
        model._chk(L.agp_svgp_predict_f(h, ptr(x), D, R, ptr(mu), ptr(var)))
        sg = torch.sqrt(var)
        z = (mu - best - xi) / sg
        Phi, phi = 0.5 * torch.erfc(-z / math.sqrt(2.0)), torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        if a.kind == "ei":
            return sg * (z * Phi + phi), Phi, phi / (2.0 * sg)
        if a.kind == "pi":
            return Phi, phi / sg, -z * phi / (2.0 * var)
        # the log kinds by the direct expressions in torch (the kindest form of the host loop; they hold down to z of about -26)
        if a.kind == "logei":
            hz = phi + z * Phi
            return torch.log(sg) + torch.log(hz), Phi / (sg * hz), phi / (2.0 * var * hz)
        return torch.log(Phi), phi / (sg * Phi), -z * phi / (2.0 * var * Phi)

    host_out = {}

    def host():
        x = X0.clamp(0.0, 1.0).contiguous()
        mo, vo, b1k, b2k = torch.zeros_like(x), torch.zeros_like(x), 1.0, 1.0
        for _ in range(T):
            _, dm, dv = ei(x)
            model._chk(L.agp_svgp_predict_f_grad(h, ptr(x), D, R, ptr(dmu), ptr(dvar), D))
            gr = dm[:, None] * dmu + dv[:, None] * dvar
            mo = b1 * mo + (1.0 - b1) * gr
            vo = b2 * vo + (1.0 - b2) * gr * gr
            b1k, b2k = b1k * b1, b2k * b2
            x = (x + lr * (mo / (1.0 - b1k)) / (torch.sqrt(vo / (1.0 - b2k)) + eps)).clamp(0.0, 1.0).contiguous()
        host_out["A"] = ei(x)[0].clone()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = (device, host)
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    enqueue.clear()
    ts = [[], []]
    for _ in range(a.reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    row = {"m": m, "D": D, "starts": R, "steps": T, "acquisition": {"ei": "EI", "pi": "PI", "logei": "LogEI", "logpi": "LogPI"}[a.kind],
           "device": stats(ts[0]), "host_loop": stats(ts[1])}
    if a.incumbent_sds:
        row["incumbent_sds"] = a.incumbent_sds
    dm_, hm_ = row["device"]["median_ms"], row["host_loop"]["median_ms"]
    row["device_us_per_step"] = round(1e3 * dm_ / (T + 1), 2)  # (T steps and the pass that evaluates the final iterate)
    row["host_loop_us_per_step"] = round(1e3 * hm_ / (T + 1), 2)
    row["ratio_host_over_device"] = round(hm_ / dm_, 3)
    row["device_enqueue_us_per_step"] = round(1e3 * float(np.median(enqueue)) / (T + 1), 2)
    row["launch_share_of_a_step"] = round(float(np.median(enqueue)) / dm_, 3)
    row["max_abs_diff_final_alpha"] = float((Ao - host_out["A"]).abs().max())
    row["checksum"] = float(Ao.sum())
    print(json.dumps({"metric": "acq_maximize_ms", "warmup": a.warmup, "reps": a.reps,
                      "timing": "device events around each call; device call and host-driven loop alternating in one process",
                      "rows": [row]}))


if __name__ == "__main__":
    main()
