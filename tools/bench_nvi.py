#!/usr/bin/env python
"""QuadratureVI (AGP_FLAG_NUMERICAL handles: the full model, or with --svgp m,B the sparse one) time per step on one GPU, one JSON line.

    python tools/bench_nvi.py [--Ns 1024,2048] [--steps 40] [--warmup 5] [--likelihood logistic] [--optimiser descent]
                              [--classical] [--nodes 100]

Per N (D = 16, SqExponential, the data of tools/bench_vgp.py): ms per agp_svgp_nvi_step, timed with device events around `steps`
steps after a warm-up (which also refreshes K), the factorisation attempts per step over the timed steps (1 + halvings: every
attempt forms a candidate, factors it and has the host read the pivot status), and next to it ms per VGP / AnalyticVI iteration
(hyper step off) of the same N and likelihood, timed as tools/bench_vgp.py does.  A step is two N^3-class products plus one
factorisation per attempt, against VGP's one factorisation with inverse.  The step waits for the host once per attempt, so the event
time includes those waits.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--Ns", default="1024,2048")
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--likelihood", default="logistic", choices=["logistic", "studentt", "laplace"])
    p.add_argument("--optimiser", default="descent", choices=["descent", "momentum", "adam"])
    p.add_argument("--classical", action="store_true", help="natural=False")
    p.add_argument("--nodes", type=int, default=100)
    p.add_argument("--no-vgp", action="store_true", help="skip the VGP iteration next to it")
    p.add_argument("--svgp", default="", help="m,B: time the sparse model SVGP with QuadratureSVI(B) on m inducing points (N = 100000, "
                   "D = 16) next to an AnalyticSVI(B) step of the same shape, instead of the full model")
    a = p.parse_args()
    import torch

    import __graft_entry__ as G

    G.build()
    import agp_amd as AGP
    from agp_amd import capi, nvi

    L = capi.lib()
    rows = []
    if a.svgp:
        return sparse(a, AGP, nvi, L, torch)
    for N in [int(n) for n in a.Ns.split(",")]:
        rng = np.random.default_rng(0)
        X = rng.random((N, 16))
        f = np.sin(3 * X[:, 0]) + X[:, 1] - 0.8
        if a.likelihood == "logistic":
            lik, y = AGP.LogisticLikelihood, (f > 0).astype(int)
        elif a.likelihood == "studentt":
            lik, y = (lambda: AGP.StudentTLikelihood(3.0, 1.0)), f + 0.2 * rng.standard_t(3, N)
        else:
            lik, y = (lambda: AGP.LaplaceLikelihood(0.4)), f + rng.laplace(0.0, 0.4, N)
        k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
        opt = {"descent": AGP.Descent(0.1), "momentum": AGP.Momentum(1e-5), "adam": AGP.ADAM(0.01)}[a.optimiser]
        row = {"N": N}
        m = AGP.VGP(X, y, k, lik(), AGP.QuadratureVI(nGaussHermite=a.nodes, optimiser=opt, natural=not a.classical), optimiser=False)
        AGP.train_(m, a.warmup)
        Xd, yd, _ = m._data
        h0 = nvi.nvi_info(m)[1]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            st = L.agp_svgp_nvi_step(m._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), None, N, 1.0)
            if st != 0:
                raise RuntimeError(L.agp_last_error(m._ctx).decode())
        e1.record()
        e1.synchronize()
        if L.agp_svgp_check_status(m._h) != 0:
            raise RuntimeError(L.agp_last_error(m._ctx).decode())
        a_last, h1, rej = nvi.nvi_info(m)
        row["step_ms"] = round(e0.elapsed_time(e1) / a.steps, 4)
        row["attempts_per_step"] = round(1.0 + (h1 - h0) / a.steps, 3)
        row["alpha_last"], row["rejected"] = a_last, rej
        row["elbo"] = round(AGP.objective(m), 4)
        del m
        if not a.no_vgp:
            v = AGP.VGP(X, y, k, lik(), AGP.AnalyticVI(), optimiser=False)
            AGP.train_(v, a.warmup)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            AGP.train_(v, a.steps)
            e1.record()
            e1.synchronize()
            row["vgp_ms"] = round(e0.elapsed_time(e1) / a.steps, 4)
            row["step_over_vgp"] = round(row["step_ms"] / row["vgp_ms"], 3)
            del v
        rows.append(row)
    print(json.dumps({"metric": "nvi_ms_per_step", "D": 16, "likelihood": a.likelihood, "optimiser": a.optimiser,
                      "natural": not a.classical, "nodes": a.nodes, "steps": a.steps,
                      "timing": "device events around the agp_svgp_nvi_step calls (host waits included)", "rows": rows}))


def sparse(a, AGP, nvi, L, torch):
    m, B = (int(v) for v in a.svgp.split(","))
    N = 100000
    rng = np.random.default_rng(0)
    X = rng.random((N, 16))
    y = (np.sin(3 * X[:, 0]) + X[:, 1] - 0.8 > 0).astype(int)
    Z = X[rng.permutation(N)[:m]].copy()
    k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(0.5)
    opt = {"descent": AGP.Descent(0.1), "momentum": AGP.Momentum(1e-5), "adam": AGP.ADAM(0.01)}[a.optimiser]
    idx = [rng.choice(N, B, replace=False) for _ in range(a.warmup + a.steps)]
    row = {"m": m, "B": B, "N": N}
    s = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.QuadratureSVI(B, nGaussHermite=a.nodes, optimiser=opt, natural=not a.classical), Z,
                 optimiser=False)
    AGP.train_(s, X, y, a.warmup, idx_stream=idx[:a.warmup])
    Xd, yd, _ = s._data
    it = [torch.as_tensor(np.asarray(i, dtype=np.int64), device=s._dev()) for i in idx[a.warmup:]]
    h0 = nvi.nvi_info(s)[1]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in it:
        st = L.agp_svgp_nvi_step(s._h, C.c_void_p(Xd.data_ptr()), Xd.stride(0), C.c_void_p(yd.data_ptr()), C.c_void_p(i.data_ptr()), B, N / B)
        if st != 0:
            raise RuntimeError(L.agp_last_error(s._ctx).decode())
    e1.record()
    e1.synchronize()
    a_last, h1, rej = nvi.nvi_info(s)
    row["step_ms"] = round(e0.elapsed_time(e1) / a.steps, 4)
    row["attempts_per_step"] = round(1.0 + (h1 - h0) / a.steps, 3)
    row["alpha_last"], row["rejected"] = a_last, rej
    del s
    if not a.no_vgp:
        v = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
        AGP.train_(v, X, y, a.warmup, idx_stream=idx[:a.warmup])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        AGP.train_(v, X, y, a.steps, idx_stream=idx[a.warmup:], state=True)
        e1.record()
        e1.synchronize()
        row["cavi_ms"] = round(e0.elapsed_time(e1) / a.steps, 4)
        row["step_over_cavi"] = round(row["step_ms"] / row["cavi_ms"], 3)
    print(json.dumps({"metric": "nvi_svgp_ms_per_step", "D": 16, "likelihood": "logistic", "optimiser": a.optimiser,
                      "natural": not a.classical, "nodes": a.nodes, "steps": a.steps,
                      "timing": "device events around the agp_svgp_nvi_step calls (host waits included); cavi_ms: train_ of "
                                "AnalyticSVI(B) on the same index stream, look-ahead on", "rows": [row]}))


if __name__ == "__main__":
    main()
