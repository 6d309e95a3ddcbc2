#!/usr/bin/env python
"""GP (exact regression, AGP_FLAG_FULL | AGP_FLAG_EXACT) per-iteration time on one GPU, one JSON line.

    python tools/bench_gp.py [--Ns 2048,4096,8192,16384] [--iters 100] [--warmup 3]

Per N (D = 16, SqExponential, opt_noise on): ms per Analytic iteration with the kernel optimiser off (noise steps only) and on
(ADAM(0.01); the hyper steps run from the fourth iteration on, as in train!), timed with device events around one train_ call of
`iters` iterations after a warm-up call (the call's fixed host cost -- the closing post_step! factorisation, status check -- is
included and spread over the iterations).  flops per iteration are counted from shapes: factorisation N^3/3 + inverse N^3/3 of
Sigma, plus N^3/3 for Sigma^-1 = L^-T L^-1 in a hyper iteration.  The CPU line is one iteration of the NumPy restatement
(tests/_gp_ref.py) at the smallest N.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--Ns", default="2048,4096,8192,16384")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    peak = C.c_double()
    rows = []
    Ns = [int(n) for n in a.Ns.split(",")]
    for N in Ns:
        rng = np.random.default_rng(0)
        X = rng.random((N, 16))
        y = np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 + 0.1 * rng.standard_normal(N)
        k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
        row = {"N": N}

        def timed(run):
            run(a.warmup)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(a.iters)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        for tag, opt in (("gp_ms", False), ("gp_hyper_ms", True)):
            m = AGP.GP(X, y, k, noise=0.01, optimiser=opt)
            row[tag] = round(timed(lambda n: AGP.train_(m, n)), 4)
            if tag == "gp_ms" and L.agp_mfma_peak(m._ensure_ctx(), capi.F64, C.byref(peak)) != 0:
                peak.value = float("nan")
            del m
        fl, flh = 2.0 * N ** 3 / 3.0, N ** 3
        nh = max(0, a.iters - 1 - max(0, 3 - a.warmup))  # hyper iterations inside the timed call (n_iter >= 3, not the last)
        flh_avg = fl + flh / 3.0 * nh / a.iters
        row["flops_per_iter"] = fl
        row["frac_mfma_peak_datasheet"] = round(fl / (row["gp_ms"] * 1e-3) / 78.6e12, 4)
        row["frac_mfma_peak_measured"] = round(fl / (row["gp_ms"] * 1e-3) / (peak.value * 1e12), 4)
        row["hyper_frac_mfma_peak_measured"] = round(flh_avg / (row["gp_hyper_ms"] * 1e-3) / (peak.value * 1e12), 4)
        rows.append(row)
    from _gp_ref import GPRef
    from oracle import agp_ref as R

    N = Ns[0]
    rng = np.random.default_rng(0)
    X = rng.random((N, 16))
    y = np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 + 0.1 * rng.standard_normal(N)
    ref = GPRef(R.Kernel("sqexponential", 0.5, 1.0), X, y, noise=0.01, construct=False)
    ref.nstate = ref.noise_opt.init(np.zeros(1))
    t0 = time.perf_counter()
    ref.step()
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"metric": "gp_ms_per_iteration", "D": 16, "timing": f"device events around train_ of {a.iters} iterations",
                      "mfma_peak_measured_tflops": round(peak.value, 2), "rows": rows,
                      "cpu_numpy_ms_per_iteration": {"N": N, "ms": round(cpu_ms, 1)}}))


if __name__ == "__main__":
    main()
