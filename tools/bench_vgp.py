#!/usr/bin/env python
"""VGP (the full variational GP, AGP_FLAG_FULL) per-iteration time on one GPU, one JSON line.

    python tools/bench_vgp.py [--Ns 2048,4096,8192] [--iters 10] [--warmup 3]

Per N (D = 16, Logistic, SqExponential): ms per CAVI iteration with the hyper step off and on (ADAM(0.01); the hyper steps run
from the fourth iteration on, as in train!), the same N for SVGP(Z = X, AnalyticVI()), timed with device events around one
train_ call of `iters` iterations after a warm-up call (the call's fixed host cost -- K refresh, status check -- is included and
spread over the iterations).  flops per iteration are counted from shapes: factorisation N^3/3 + inverse N^3/3 of -2 eta2 for VGP;
SVGP with m = B = N adds the symmetric product kappa' diag(theta) kappa (N^3) and W = kappa L^-T (N^3).  The CPU line is one
iteration of the NumPy restatement (tests/_vgp_ref.py) at the smallest N.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--Ns", default="2048,4096,8192")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--svgp-max", type=int, default=4096, help="largest N of the SVGP(Z = X) comparison")
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi
    import ctypes as C

    L = capi.lib()
    peak = C.c_double()
    rows = []
    Ns = [int(n) for n in a.Ns.split(",")]
    for N in Ns:
        rng = np.random.default_rng(0)
        X = rng.random((N, 16))
        y = (np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 > 0).astype(int)
        k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
        row = {"N": N}

        def timed(model, run):
            run(a.warmup)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(a.iters)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        for tag, opt in (("vgp_ms", False), ("vgp_hyper_ms", True)):
            m = AGP.VGP(X, y, k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=opt)
            row[tag] = round(timed(m, lambda n: AGP.train_(m, n)), 4)
            if tag == "vgp_ms" and L.agp_mfma_peak(m._ensure_ctx(), capi.F64, C.byref(peak)) != 0:
                peak.value = float("nan")
            del m
        if N <= a.svgp_max:
            m = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), X.copy(), optimiser=False)
            row["svgp_z_eq_x_ms"] = round(timed(m, lambda n: AGP.train_(m, X, y, n)), 4)
            row["speedup"] = round(row["svgp_z_eq_x_ms"] / row["vgp_ms"], 3)
            del m
        fl = 2.0 * N ** 3 / 3.0
        row["flops_per_iter"] = fl
        row["frac_mfma_peak_datasheet"] = round(fl / (row["vgp_ms"] * 1e-3) / 78.6e12, 4)
        row["frac_mfma_peak_measured"] = round(fl / (row["vgp_ms"] * 1e-3) / (peak.value * 1e12), 4)
        rows.append(row)
    # the CPU line: one iteration of the restatement
    from _vgp_ref import VGPRef
    from oracle import agp_ref as R

    N = Ns[0]
    rng = np.random.default_rng(0)
    X = rng.random((N, 16))
    yt = np.where(np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 > 0, 1.0, -1.0)
    ref = VGPRef(R.Kernel("sqexponential", 0.5, 1.0), R.LogisticLikelihood(), X)
    t0 = time.perf_counter()
    ref.step(yt)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"metric": "vgp_ms_per_iteration", "D": 16, "likelihood": "logistic", "timing": "device events around "
                      f"train_ of {a.iters} iterations", "mfma_peak_measured_tflops": round(peak.value, 2), "rows": rows,
                      "cpu_numpy_ms_per_iteration": {"N": N, "ms": round(cpu_ms, 1)}}))


if __name__ == "__main__":
    main()
