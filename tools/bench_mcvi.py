#!/usr/bin/env python
"""The Monte-Carlo expectation kernel of MCIntegrationVI on given moments (agp_mc_expectations: k_mc_normals + k_mc_local), timed.

    python tools/bench_mcvi.py [--B 1024] [--K 8] [--nMC 1000] [--reps 20] [--link softmax|logisticsoftmax]
    rocprofv3 --kernel-trace --stats -- python tools/bench_mcvi.py        (the per-kernel times DESIGN.md section 9j records)

Prints the wall time per call (which includes the table's allocation, the upload of nothing and one synchronisation) as a JSON
line; the kernels' own times come from the trace.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--nMC", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--link", default="softmax")
    a = ap.parse_args()
    import numpy as np
    import torch

    import agp_amd as AGP

    rng = np.random.default_rng(0)
    mu, var = rng.standard_normal((a.K, a.B)), rng.uniform(0.1, 2.0, (a.K, a.B))
    c = rng.integers(0, a.K, a.B)
    lik = AGP.SoftMaxLikelihood(a.K) if a.link == "softmax" else AGP.LogisticSoftMaxLikelihood(a.K)
    AGP.mc_expectations(lik, c, mu, var, a.nMC, 1, 1)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(a.reps):
        ell, g, h = AGP.mc_expectations(lik, c, mu, var, a.nMC, 1, 2 + r)
    dt = (time.perf_counter() - t0) / a.reps
    print(json.dumps(dict(B=a.B, K=a.K, nMC=a.nMC, link=a.link, exps_per_call=a.B * a.nMC * a.K, wall_ms_per_call=1e3 * dt,
                          ell_mean=float(np.mean(ell)))))


if __name__ == "__main__":
    main()
