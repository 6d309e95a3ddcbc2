#!/usr/bin/env python
"""SHA-256 hashes of results that cross every path of the tile factorisation's 4-column rounds (chol_rounds, csrc/agp_chol.h):

    python tools/round_layout_golden.py            # print the hashes of the library in use
    python tools/round_layout_golden.py --write [FILE]   # ... and store them (default: tests/golden/round_layout_hashes.json)

* the factor that agp_potrf_jitter (jitter 0) returns for A = G G' / n + I / 2 (G n x (n + 8), seeded by n), n = 64, 96, 200, in fp64
  and fp32 (the recipe of tests/test_gpu_tile_rounds.py);
* mu, Sigma (get_state) and the ELBO (float.hex) of an SVGP, SqExponential + Logistic, after 5 CAVI steps: m = 128 / 192 inducing
  points (2 / 3 block columns), batches of 64 / 200 (one full tile / a ragged one), D = 4, N = 2000; get_state takes the pending
  step through flush().

tests/test_gpu_round_layout.py compares the library under test with the stored file, bit for bit.  The file is written from the
build of the commit BEFORE a change that must leave the arithmetic alone (AGP_HIP_LIB selects that build), on an MI355X, and is
regenerated only by a change that alters arithmetic on purpose."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "round_layout_hashes.json")
POTRF_N = (64, 96, 200)
SVGP_CASES = ((128, 64), (128, 200), (192, 64), (192, 200))  # (m, B)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def spd(n):
    G = np.random.default_rng(n).standard_normal((n, n + 8))
    return G @ G.T / n + 0.5 * np.eye(n)


def potrf_hash(n, dt):
    """sha256 of the n x n array that agp_potrf_jitter leaves (dt 0: fp64, 1: fp32)"""
    import torch
    from agp_amd import capi

    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        ad = torch.tensor(spd(n), dtype=torch.float32 if dt else torch.float64, device="cuda").contiguous()
        info = C.c_int32(-7)
        st = L.agp_potrf_jitter(ctx, dt, C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        torch.cuda.synchronize()
        assert st == 0 and info.value == 0, (st, info.value)
        return _sha(ad.cpu().numpy())
    finally:
        L.agp_ctx_destroy(ctx)


def svgp_hashes(m, B):
    """{"mu": sha256, "Sigma": sha256, "elbo": float.hex} after 5 CAVI steps"""
    import agp_amd as AGP

    rng = np.random.default_rng(1000 * m + B)
    N, D, iters = 2000, 4, 5
    X = rng.random((N, D))
    y = np.sign(np.sin(4 * X[:, 0]) + X[:, 1] - 0.8 + 0.3 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    k = AGP.SqExponentialKernel() @ AGP.ScaleTransform(2.0)
    model = AGP.SVGP(k, AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
    AGP.train_(model, X, y, iters, idx_stream=idx)
    mu, Sig, _, _ = model.get_state(0)
    elbo = AGP.ELBO(model, X[:B], y[:B])
    return {"mu": _sha(mu), "Sigma": _sha(Sig), "elbo": float(elbo).hex()}


def compute():
    out = {}
    for dt, dn in ((0, "f64"), (1, "f32")):
        for n in POTRF_N:
            out[f"potrf_{dn}_n{n}"] = potrf_hash(n, dt)
    for m, B in SVGP_CASES:
        out[f"svgp_m{m}_B{B}"] = svgp_hashes(m, B)
    return out


if __name__ == "__main__":
    import __graft_entry__ as g

    g.build()
    res = compute()
    print(json.dumps(res, indent=1, sort_keys=True))
    if "--write" in sys.argv[1:]:
        rest = sys.argv[sys.argv.index("--write") + 1:]
        path = os.path.abspath(rest[0]) if rest else GOLDEN
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("->", path)
