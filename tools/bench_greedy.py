"""Times the greedy conditional-variance selection (agp_greedy_variance) at the C2 size -- N = 1e6, D = 32, m = 1024, fp64 -- with
HIP events around the call, and prints the achieved bytes/s against the HBM rate of the MI355X (8.0 TB/s datasheet, 6.29 TB/s
measured with a float4 copy) and the k-means selection (`inducingpoints(KmeansAlg(m), X)`) at the same size beside it.

    python tools/bench_greedy.py [--N 1000000] [--D 32] [--m 1024] [--scale 0.5] [--reps 3] [--no-kmeans]

Bytes counted per call: step j reads j columns of the factor and D columns of X, reads and writes the residual and writes one
column, all of N doubles: 8 N (m (m - 1) / 2 + m (D + 3)).  The one-off transpose of X, the zero-fill of the factor (8 N m) and the
optional n x m output copy are inside the timed call but not in the byte count.  A record, not a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as g

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kmeans", action="store_true")
    a = ap.parse_args()
    g.build()
    import agp_amd as AGP
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    N, D, m = a.N, a.D, a.m
    X = torch.rand(N, D, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    kern = AGP.SqExponentialKernel() @ AGP.ScaleTransform(a.scale)
    kd, keep = kern.desc(D)
    idx = torch.empty(m, dtype=torch.int64, device="cuda")
    Z = torch.empty(m, D, dtype=torch.float64, device="cuda")
    tr = torch.empty(m, dtype=torch.float64, device="cuda")
    nsel = C.c_int64()
    ms = []
    for rep in range(a.reps + 1):  # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = L.agp_greedy_variance(ctx, capi.F64, C.byref(kd), X.data_ptr(), N, D, D, m, 1e-9, idx.data_ptr(), Z.data_ptr(), D, None,
                                   0, tr.data_ptr(), C.byref(nsel))
        e1.record()
        e1.synchronize()
        assert st == 0, L.agp_last_error(ctx)
        if rep:
            ms.append(e0.elapsed_time(e1))
    t = min(ms) * 1e-3
    nbytes = 8.0 * N * (m * (m - 1) / 2 + m * (D + 3))
    trace = tr.cpu().numpy()
    res = dict(bench="greedy_variance", N=N, D=D, m=m, scale=a.scale, selected=int(nsel.value), ms=[round(v, 3) for v in ms],
               best_ms=round(t * 1e3, 3), us_per_step=round(t * 1e6 / max(int(nsel.value), 1), 2), bytes=nbytes,
               tb_per_s=round(nbytes / t / 1e12, 3), frac_hbm_spec=round(nbytes / t / HBM_SPEC, 3),
               frac_hbm_copy=round(nbytes / t / HBM_COPY, 3), trace_first=float(trace[0]), trace_last=float(trace[int(nsel.value) - 1]))
    if not a.no_kmeans:
        ts = []
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = AGP.inducingpoints(AGP.KmeansAlg(m), X, rng=np.random.default_rng(0), return_info=True)
            ts.append(time.perf_counter() - t0)
        res.update(kmeans_ms=round(min(ts) * 1e3, 1), kmeans_iterations=info["iterations"], kmeans_converged=info["converged"])
    L.agp_ctx_destroy(ctx)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
