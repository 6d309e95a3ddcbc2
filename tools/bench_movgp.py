#!/usr/bin/env python
"""MOVGP (the multi-output full variational GP) per-iteration time on one GPU, one JSON line.

    python tools/bench_movgp.py [--Ns 2048,4096] [--Qs 2,4] [--iters 100] [--warmup 3]

Per (N, Q) (D = 16, tasks Logistic + Laplace(2), SqExponential, Aoptimiser ADAM(0.01), hyper step off): ms per iteration, timed with
device events around one train_ call of `iters` iterations after a warm-up call, and -- unless --no-vgp -- the same timing of a
VGP (Logistic) at the same N with the ratio movgp_ms / (Q * vgp_ms): the Q factorisations with inverse run one after another, so a
ratio near 1 is the expectation.  The reference's multi-output step can diverge (section 9g), and nobody has
checked these sizes: the status and the objective are read after the timed call, and a run whose objective is not finite is
reported as such ("finite": false) with no time.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--Ns", default="2048,4096")
    p.add_argument("--Qs", default="2,4")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-vgp", action="store_true")
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP

    def timed(run):
        run(a.warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(a.iters)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    rows = []
    for N in [int(n) for n in a.Ns.split(",")]:
        rng = np.random.default_rng(0)
        X = rng.random((N, 16))
        f = np.sin(3 * X[:, 0]) + X[:, 1] - 0.8
        f2 = np.cos(4 * X[:, 1])
        ys = [(f > 0).astype(int), f2 + rng.laplace(0.0, 0.3, N)]
        k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
        vgp_ms = None
        if not a.no_vgp:
            m = AGP.VGP(X, ys[0], k, AGP.LogisticLikelihood(), AGP.AnalyticVI(), optimiser=False)
            vgp_ms = timed(lambda n: AGP.train_(m, n))
            del m
        for Q in [int(q) for q in a.Qs.split(",")]:
            m = AGP.MOVGP(X, ys, k, [AGP.LogisticLikelihood(), AGP.LaplaceLikelihood(2.0)], AGP.AnalyticVI(), Q, optimiser=False,
                          Aoptimiser=AGP.ADAM(0.01), seed=0)
            row = {"N": N, "Q": Q}
            try:
                ms = timed(lambda n: AGP.train_(m, n))  # (train_ ends with the handle's status check)
                obj = AGP.objective(m)
                row["status"] = "ok"
            except AGP.AGPError as e:
                ms, obj = None, float("nan")
                row["status"] = str(e)
            row["objective"] = obj if math.isfinite(obj) else None
            row["finite"] = bool(math.isfinite(obj))
            if row["finite"] and ms is not None:
                row["movgp_ms"] = round(ms, 4)
                if vgp_ms is not None:
                    row["vgp_ms"] = round(vgp_ms, 4)
                    row["ratio_to_Q_vgp"] = round(ms / (Q * vgp_ms), 3)
            rows.append(row)
            del m
    print(json.dumps({"metric": "movgp_ms_per_iteration", "D": 16, "tasks": "logistic+laplace(2)", "Aoptimiser": "ADAM(0.01)",
                      "timing": f"device events around train_ of {a.iters} iterations", "rows": rows}))


if __name__ == "__main__":
    main()
