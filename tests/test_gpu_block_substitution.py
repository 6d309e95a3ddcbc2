"""The CAVI step's task-graph launches hand the tile inverse over without its off-diagonal block (DESIGN.md sections 4, 5, 12):
the slot of block column k holds [[X11, 0], [L21, X22]] and every product T X_k' -- the chain's L(k+1, k) and the panel and
extension-row tiles -- is a forward substitution in two 32-column blocks.  Launches with identity rows (get_state, ELBO, prediction)
keep the full inverse.  The summation order changes against the plain product, so the checks are against the oracle with the CAVI
step's tolerances (1e-9 on eta, 1e-8 on mu and Sigma), across the gate on one handle, bitwise between the merged and the split
launch, and on the tile factorisation alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


# ---------------------------------------------------------------------------------------------------------------------------------
# the algebra and the slot format (no device)
def test_three_stage_substitution_equals_the_product_with_the_inverse():
    rng = np.random.default_rng(3)
    for _ in range(8):
        G = rng.standard_normal((64, 96))
        A = G @ G.T / 96 + 0.5 * np.eye(64)
        T = rng.standard_normal((64, 64))
        L = np.linalg.cholesky(A)
        L11, L21, L22 = L[:32, :32], L[32:, :32], L[32:, 32:]
        slot = np.zeros((64, 64))  # [[X11, 0], [L21, X22]]
        slot[:32, :32] = np.linalg.inv(L11)
        slot[32:, :32] = L21
        slot[32:, 32:] = np.linalg.inv(L22)
        L1 = T[:, :32] @ slot[:32, :32].T
        U = T[:, 32:] - L1 @ slot[32:, :32].T
        L2 = U @ slot[32:, 32:].T
        got = np.hstack([L1, L2])
        want = T @ np.linalg.inv(L).T
        assert _rel(got, want) <= 1e-13
        assert np.all(slot[:32, 32:] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
def _problem(seed, N, D, m, B, iters):
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
    y = np.sign(f + 0.3 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    return X, y, Z, idx


def _models(Z, B):
    import agp_amd as AGP
    from oracle import agp_ref as R

    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                  optimiser=False)
    mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
    return AGP, ma, mr


def _check_state(ma, mr):
    g = mr.latents[0]
    mu, Sig, e1, e2 = ma.get_state(0)
    errs = (_rel(e1, g.eta1), _rel(e2, g.eta2), _rel(mu, g.mu), _rel(Sig, g.Sigma))
    print("eta1 %.2e  eta2 %.2e  mu %.2e  Sigma %.2e" % errs)
    assert errs[0] <= 1e-9 and errs[1] <= 1e-9
    assert errs[2] <= 1e-8 and errs[3] <= 1e-8


def _prologues(ma):
    from agp_amd import capi

    ns, npro = C.c_int64(), C.c_int64()
    ma._chk(capi.lib().agp_svgp_step_counters(ma._h, C.byref(ns), C.byref(npro)))
    return ns.value, npro.value


# m = 128: two block columns, the smallest chain with feeders; m = 100: padded last tile (nvalid < mp); m = 1024: 16 columns
@pytest.mark.gpu
@pytest.mark.parametrize("m,B", [(128, 64), (192, 128), (100, 70), (1024, 64)])
def test_trajectory_matches_oracle(built, m, B):
    iters = 5
    X, y, Z, idx = _problem(21 + m, 1500, 4, m, B, iters)
    AGP, ma, mr = _models(Z, B)
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    mr.train(X, y, iters, idx_stream=idx)
    _check_state(ma, mr)


@pytest.mark.gpu
def test_steps_and_launches_with_identity_rows_alternate_on_one_handle(built):
    """step launches (slots without X21) -> get_state / ELBO / predict_f (full inverse) -> step launches again"""
    m, B, iters = 192, 128, 4
    X, y, Z, idx = _problem(5, 1500, 4, m, B, 2 * iters)
    AGP, ma, mr = _models(Z, B)
    AGP.train_(ma, X, y, iters, idx_stream=idx[:iters])
    mr.train(X, y, iters, idx_stream=idx[:iters])
    _check_state(ma, mr)
    hid = lambda: getattr(ma._h, "value", ma._h)
    h0, npro0 = hid(), _prologues(ma)[1]
    assert npro0 >= iters - 2  # the pending step rode on the step launches
    # (evaluation batches within the handle's batch size: a larger one would make the model build a new handle)
    ea, er = AGP.ELBO(ma, X[:B], y[:B], rho=1.0), mr.elbo_fresh(X[:B], y[:B], 1.0)
    assert ea == pytest.approx(er, rel=1e-8)
    Xt = X[:77]
    pm, pv = AGP.predict_f(ma, Xt, cov=True)
    rm, rv = mr.predict_f(Xt, cov=True)
    assert _rel(pm, rm[0]) <= 1e-8 and _rel(pv, rv[0]) <= 1e-8
    AGP.train_(ma, X, y, iters, idx_stream=idx[iters:], state=True)
    mr.train(X, y, iters, idx_stream=idx[iters:], fresh_state=False)
    _check_state(ma, mr)
    nsteps, npro = _prologues(ma)
    print("steps", nsteps, "with prologue", npro0, "then", npro)
    assert hid() == h0  # one handle throughout
    assert npro - npro0 >= iters - 2  # ... and again behind the launches with identity rows


_SPLIT_CODE = r"""
import numpy as np, hashlib, sys
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import agp_amd as AGP
rng = np.random.default_rng(8)
N, D, m, B, iters = 1500, 4, 256, 128, 10
X = rng.random((N, D)); f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
y = np.sign(f + 0.3 * rng.standard_normal(N))
Z = X[rng.permutation(N)[:m]].copy()
idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
model = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
AGP.train_(model, X, y, iters, idx_stream=idx)
mu, Sig, e1, e2 = model.get_state(0)
print('HASH', hashlib.sha256(np.ascontiguousarray(e2).tobytes() + np.ascontiguousarray(e1).tobytes()).hexdigest())
"""


@pytest.mark.gpu
def test_split_launch_is_bitwise_the_merged_launch(built):
    """chain kernel + tile kernel read the same slot format as the merged kernel: eta after 10 steps is bit-identical"""
    hashes = []
    for split in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", _SPLIT_CODE], cwd=ROOT, env=dict(os.environ, AGP_CHAIN_SPLIT=split),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        hashes.append([l for l in r.stdout.splitlines() if l.startswith("HASH")][0])
    assert hashes[0] == hashes[1]


@pytest.mark.gpu
def test_tile_factorisation_without_x21_passes_its_residual_check(built):
    """agp_dev_diag_bench variant 13 (fp64; the substitution is not enabled for fp32): |L L' - A|, |X11 L11 - I|, |X22 L22 - I|
    below 1e-12, the L21 block of the slot exact, nothing above the diagonal"""
    import torch
    from agp_amd import capi

    L = capi.lib()
    f = L.agp_dev_diag_bench
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        for blocks in (1, 16):
            us = C.c_double()
            assert f(ctx, 0, 13, blocks, 4, C.byref(us)) == 0
            assert f(ctx, 0, 1, blocks, 4, C.byref(us)) == 0  # the full inverse next to it
    finally:
        L.agp_ctx_destroy(ctx)
