#!/usr/bin/env python
"""MCGP (Gibbs sampling of the augmented full GP, AGP_FLAG_FULL | AGP_FLAG_SAMPLED) time per sweep on one GPU, one JSON line.

    python tools/bench_mcgp.py [--Ns 1024,2048,4096] [--sweeps 40] [--warmup 5] [--likelihood logistic]

Per N (D = 16, SqExponential, the data of tools/bench_vgp.py): ms per Gibbs sweep, timed with device events around one `sample`
call of `sweeps` sweeps that keeps only the last one, after a warm-up call (which also refreshes K); next to it ms per VGP iteration
(hyper step off) of the same N and likelihood, timed as tools/bench_vgp.py does, and their ratio.  A sweep does VGP's factorisation
and replaces the column-statistics pass by one triangular product and the variate draws.  `host_enqueue_ms` is the host time of the
timed `sample` call up to its return from agp_svgp_gibbs_sample's enqueue (the call itself ends with a status check, which waits).
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--Ns", default="1024,2048,4096")
    p.add_argument("--sweeps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--likelihood", default="logistic", choices=["logistic", "studentt", "negbinomial"])
    p.add_argument("--no-vgp", action="store_true", help="skip the VGP iteration next to it")
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    rows = []
    for N in [int(n) for n in a.Ns.split(",")]:
        rng = np.random.default_rng(0)
        X = rng.random((N, 16))
        f = np.sin(3 * X[:, 0]) + X[:, 1] - 0.8
        if a.likelihood == "logistic":
            lik, y = AGP.LogisticLikelihood, (f > 0).astype(int)
        elif a.likelihood == "studentt":
            lik, y = (lambda: AGP.StudentTLikelihood(3.0, 1.0)), f + 0.2 * rng.standard_t(3, N)
        else:
            lik, y = (lambda: AGP.NegBinomialLikelihood(6.0)), rng.negative_binomial(6, 1.0 / (1.0 + np.exp(f)))
        k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
        row = {"N": N}
        m = AGP.MCGP(X, y, k, lik(), AGP.GibbsSampling(nBurnin=0))
        AGP.sample(m, 1, discard_initial=a.warmup - 1, seed=1)
        yd = m._data[1]
        store = torch.empty(1, N, dtype=torch.float64, device=m._dev())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        st = L.agp_svgp_gibbs_sample(m._h, C.c_void_p(yd.data_ptr()), 1, a.sweeps - 1, 1, C.c_uint64(1), C.c_void_p(store.data_ptr()), N)
        row["host_enqueue_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        e1.record()
        e1.synchronize()
        if st != 0 or L.agp_svgp_check_status(m._h) != 0:
            raise RuntimeError(L.agp_last_error(m._ctx).decode())
        row["sweep_ms"] = round(e0.elapsed_time(e1) / a.sweeps, 4)
        del m
        if not a.no_vgp:
            v = AGP.VGP(X, y, k, lik(), AGP.AnalyticVI(), optimiser=False)
            AGP.train_(v, a.warmup)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            AGP.train_(v, a.sweeps)
            e1.record()
            e1.synchronize()
            row["vgp_ms"] = round(e0.elapsed_time(e1) / a.sweeps, 4)
            row["sweep_over_vgp"] = round(row["sweep_ms"] / row["vgp_ms"], 3)
            del v
        rows.append(row)
    print(json.dumps({"metric": "mcgp_ms_per_sweep", "D": 16, "likelihood": a.likelihood, "sweeps": a.sweeps,
                      "timing": "device events around one agp_svgp_gibbs_sample call", "rows": rows}))


if __name__ == "__main__":
    main()
