"""The fp64 MFMA operand reads of the Cholesky kernels (lds_keep_apart64 in mma8, mma8_sub, mma_blk32, mma_tile16 and
mma_tile16_chain, agp_chol.h; DESIGN.md section 5 "round 15"): since round 15 every fp64 operand is read by a ds_read_b64 of its own
instead of sharing a ds_read2_b64 with the operand of the neighbouring k-step.  Same operands, same LDS addresses, same MFMA order per
accumulator, same summation order: every bit of every path must be what the parent commit computed, and the float kernels are the
parent's instruction for instruction.  tests/test_gpu_subst_readahead.py, tests/test_gpu_chain_product_balance.py and
tests/test_gpu_round_layout.py already pin the CAVI step's single-latent launch; this file pins the paths that had no pin:

* agp_potrf_jitter, fp64, jitter 0, n = 128, 136, 320 on the matrices of tests/test_gpu_chain_product_balance.py (G G' / n + I / 2,
  G n x (n + 8), seeded by n): a factor launch without the step (mma_tile16's loop, the full-inverse glue, both TB forms of
  mma_blk32), and again with AGP_CHOL_DAG=0 (k_chol_step).  SHA-256 of L, and ||L L' - A|| / ||A|| (max norm) <= 4 n u.
  (These three A come out of numpy's matmul, as in that file: their pins hold for the BLAS the hashes were recorded with.)
* n = 6144, fp64, default settings: the smallest size on the blocked path (k_chol_panel / k_chol_trail).  So that the pinned hash
  depends on no BLAS, the matrix is the same family with G rounded to multiples of 1/4: G G' is then exact in fp64 in any summation
  order (it is formed on the device), and / n + I / 2 rounds once per element.  SHA-256 of L; the residual by a float64 matmul on the
  device with the same 4 n u bound.
* the batched step launch: SVGP with LogisticSoftMaxLikelihood(3), m = 128, B = 64, D = 4, N = 1500, 3 steps.  SHA-256 over
  (mu, Sigma, eta1, eta2) of the three latents, merged = split launch, and the CPU oracle with the tolerances of
  tests/test_gpu_feeder_split.py (1e-9 on eta, 1e-8 on mu and Sigma).
* the hyper iteration: Logistic SVGP with optimiser=ADAM(0.01), m = 128, B = 64, three hyper iterations (identity rows, product
  workgroups).  train_ takes its first hyper step behind the third CAVI step and none behind the last, so three hyper iterations
  are six calls of the train loop.  SHA-256 over the state, the kernel parameters and the inducing points.
* Logistic SVGP, 5 steps at (m, B) = (448, 100): seven block columns, feeders on the prefetched path.  SHA-256, merged = split, oracle.
* fp32: agp_potrf_jitter at n = 136 in float.  The float code object is the parent's, so this holds trivially -- and fails if a float
  kernel was touched after all.

One child process per setting (the levers are read once per process).  Under a fallback-forcing variable (tests/_knobs.py) only the
numerical comparisons apply."""
import os
import subprocess
import sys

import pytest

import _knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53

# What the commit before round 15 (cc2e6d0, "Add joint Monte-Carlo batch acquisition (q-EI, q-UCB) on the device") printed for _RUN
# below on an MI355X.  Round 15 splits LDS reads and nothing else, so these hold as long as no operand, no MFMA order and no
# summation order of these paths changes; a pull request that changes one of those on purpose re-pins them and says so.
PARENT = {
    "default": {
        "potrf64_128": "40bd3a00920e187341a88c59de23107db34d1ebcbd668df255c905d2e6b8a278",
        "potrf64_136": "bd39e78a299cb784289312d1a4ba1336aabfa75edcbfe3f1b82e35c742df2565",
        "potrf64_320": "40b1b9a3d3785e24ffbfead3a48595323056aec4516cbb55ba4bf6ddaa1b65ca",
        "potrf32_136": "478b0556b4528312b5a3525b8146ed102f93dcfcb9d51725d16b1894be950a7e",
        "potrf64_6144": "ff2e00a6212cf6153b4525969c2ffb7de0a63e1a1d6593c1fd400c23d0c0c67c",
        "softmax": "b24107014ff21a94700d6a9ad951a5f848628d3faceaed6b61fc4df51ccc3c49",
        "hyper": "a3910a26a90f0475b982d5efe1d3a6b26b8ca08b8f8aa99a5bd98bdf7bc8c4b3",
        "svgp448": "978af5ae6f2d6923bdbc850f6f6405d0e56e075c9096f3bed002eb7df51e9638",
    },
    "nodag": {  # AGP_CHOL_DAG=0
        "potrf64_128": "f1d4a9ce99a25834bff7baca68cb6ec9771cbee700a058500e789e0e21490efe",
        "potrf64_136": "75c48f90560604fc41d149b64d27a7c65b78cd66133843bbe4c0ddd219f5703e",
        "potrf64_320": "0d99d85b6c621093a0b600760ce89b95543521a25e15fec00432b6fa7d6ee492",
    },
}

_RUN = r"""
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import torch
import agp_amd as AGP
from agp_amd import capi
from oracle import agp_ref as R
what = sys.argv[1:]
sha = lambda *arrs: hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in arrs)).hexdigest()
rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))

def potrf(ad, prec):
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        n = ad.shape[0]
        info = C.c_int32(-7)
        st = L.agp_potrf_jitter(ctx, prec, C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        torch.cuda.synchronize()
        assert st == 0 and info.value == 0, (st, info.value)
    finally:
        L.agp_ctx_destroy(ctx)

if 'potrf' in what:
    for prec, dt, sizes in ((0, torch.float64, (128, 136, 320)), (1, torch.float32, (136,))):
        for n in sizes:
            G = np.random.default_rng(n).standard_normal((n, n + 8))
            A = G @ G.T / n + 0.5 * np.eye(n)
            ad = torch.tensor(A, dtype=dt, device='cuda').contiguous()
            A = ad.cpu().numpy().astype(np.float64)
            potrf(ad, prec)
            Lf = np.tril(ad.cpu().numpy())
            L64 = Lf.astype(np.float64)
            print('HASH', 'potrf%d_%d' % (64 if prec == 0 else 32, n), sha(Lf))
            print('RES', 'potrf%d_%d' % (64 if prec == 0 else 32, n), float(np.abs(L64 @ L64.T - A).max() / np.abs(A).max()))

if 'blocked' in what:
    n = 6144
    G = np.rint(4.0 * np.random.default_rng(n).standard_normal((n, n + 8))) / 4.0
    Gd = torch.tensor(G, dtype=torch.float64, device='cuda')
    Ad = Gd @ Gd.T / n + 0.5 * torch.eye(n, dtype=torch.float64, device='cuda')  # G G' exact: multiples of 1/16 far below 2^53
    del Gd
    ad = Ad.clone().contiguous()
    potrf(ad, 0)
    Ld = torch.tril(ad)
    print('HASH', 'potrf64_6144', sha(Ld.cpu().numpy()))
    print('RES', 'potrf64_6144', float(((Ld @ Ld.T - Ad).abs().max() / Ad.abs().max()).item()))

def data(seed, m, B, iters, N=1500, D=4):
    rng = np.random.default_rng(seed)
    X = rng.random((N, D)); f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
    noisy = f + 0.3 * rng.standard_normal(N)
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    return X, noisy, Z, idx

def state(ma):
    out = []
    for k in range(ma.n_latent):
        out += list(ma.get_state(k))
    return out

def oracle_err(name, ma, mr):
    e = [0.0] * 4
    for k in range(ma.n_latent):
        mu, Sig, e1, e2 = ma.get_state(k)
        gr = mr.latents[k]
        for i, (a, b) in enumerate(((e2, gr.eta2), (e1, gr.eta1), (mu, gr.mu), (Sig, gr.Sigma))):
            e[i] = max(e[i], rel(a, b))
    print('ERR', name, *e)

if 'softmax' in what:
    m, B, iters = 128, 64, 3
    X, noisy, Z, idx = data(15 + m + B, m, B, iters)
    y = 1 + np.digitize(noisy, np.quantile(noisy, [0.33, 0.66]))
    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(B), Z, optimiser=False)
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    assert ma.n_latent == 3
    print('HASH', 'softmax', sha(*state(ma)))
    if 'oracle' in what:
        mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticSoftMaxLikelihood(3), Z, stochastic=True, batchsize=B)
        mr.train(X, y, iters, idx_stream=idx)
        oracle_err('softmax', ma, mr)

if 'hyper' in what:
    m, B, iters = 128, 64, 6  # hyper steps behind CAVI steps 3, 4 and 5
    X, noisy, Z, idx = data(16 + m + B, m, B, iters)
    y = np.sign(noisy)
    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=AGP.ADAM(0.01))
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    var, sc = C.c_double(), (C.c_double * 4)()
    ma._chk(capi.lib().agp_svgp_get_kernel(ma._h, 0, C.byref(var), sc))
    kp = np.array([var.value] + list(sc))
    print('KERNEL', 'hyper', *kp)
    print('HASH', 'hyper', sha(*state(ma), kp, np.asarray(ma.Zs[0])))

if 'svgp448' in what:
    m, B, iters = 448, 100, 5
    X, noisy, Z, idx = data(15 + m + B, m, B, iters)
    y = np.sign(noisy)
    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    print('HASH', 'svgp448', sha(*state(ma)))
    if 'oracle' in what:
        mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
        mr.train(X, y, iters, idx_stream=idx)
        oracle_err('svgp448', ma, mr)
"""

_SETTINGS = {
    "default": ({}, ("potrf", "blocked", "softmax", "hyper", "svgp448", "oracle")),
    "nodag": ({"AGP_CHOL_DAG": "0"}, ("potrf",)),
    "merged": ({"AGP_CHAIN_SPLIT": "0"}, ("softmax", "svgp448")),
    "split": ({"AGP_CHAIN_SPLIT": "1"}, ("softmax", "svgp448")),
}
_cache = {}


def _run(key):
    """one process per setting; shared by the tests below"""
    if key not in _cache:
        env_extra, what = _SETTINGS[key]
        r = subprocess.run([sys.executable, "-c", _RUN, *what], cwd=ROOT, env=dict(os.environ, **env_extra), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w and w[0] == "HASH":
                out[("hash", w[1])] = w[2]
            elif w and w[0] == "RES":
                out[("res", w[1])] = float(w[2])
            elif w and w[0] == "ERR":
                out[("err", w[1])] = tuple(float(v) for v in w[2:6])
            elif w and w[0] == "KERNEL":
                out[("kernel", w[1])] = tuple(float(v) for v in w[2:])
        _cache[key] = out
    return _cache[key]


def _bitwise():
    return not _knobs.forced(*_knobs._DEFAULTS)


def _check_oracle(out, name):
    e_eta2, e_eta1, e_mu, e_sig = out[("err", name)]
    print(f"{name}: eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}  sha256 {out[('hash', name)]}")
    assert e_eta2 <= 1e-9 and e_eta1 <= 1e-9
    assert e_mu <= 1e-8 and e_sig <= 1e-8


@pytest.mark.parametrize("setting", ["default", "nodag"])
@pytest.mark.parametrize("n", [128, 136, 320])
def test_potrf_fp64_residual_and_the_parent_bit_for_bit(built, n, setting):
    out = _run(setting)
    name = f"potrf64_{n}"
    res = out[("res", name)]
    print(f"{setting}, n = {n}: residual {res:.3e} (bound {4 * n * U:.3e})  sha256 {out[('hash', name)]}")
    assert res <= 4 * n * U, (res, 4 * n * U)
    if _bitwise():
        assert out[("hash", name)] == PARENT[setting][name]


def test_blocked_potrf_fp64_residual_and_the_parent_bit_for_bit(built):
    out, n = _run("default"), 6144
    res = out[("res", "potrf64_6144")]
    print(f"n = {n}: residual {res:.3e} (bound {4 * n * U:.3e})  sha256 {out[('hash', 'potrf64_6144')]}")
    assert res <= 4 * n * U, (res, 4 * n * U)
    if _bitwise():
        assert out[("hash", "potrf64_6144")] == PARENT["default"]["potrf64_6144"]


def test_potrf_fp32_is_the_parent_bit_for_bit(built):
    out, n = _run("default"), 136
    res = out[("res", "potrf32_136")]
    print(f"float, n = {n}: residual {res:.3e} (bound {4 * n * 2.0 ** -24:.3e})  sha256 {out[('hash', 'potrf32_136')]}")
    assert res <= 4 * n * 2.0 ** -24
    if _bitwise():
        assert out[("hash", "potrf32_136")] == PARENT["default"]["potrf32_136"]


@pytest.mark.parametrize("name", ["softmax", "svgp448"])
def test_step_launches_match_oracle_and_the_parent_bit_for_bit(built, name):
    out = _run("default")
    _check_oracle(out, name)
    if _bitwise():
        assert out[("hash", name)] == PARENT["default"][name]


@pytest.mark.parametrize("name", ["softmax", "svgp448"])
def test_split_launch_is_bitwise_the_merged_launch(built, name):
    merged, split = _run("merged"), _run("split")
    print(f"{name}: merged {merged[('hash', name)]}  split {split[('hash', name)]}")
    if _bitwise():
        assert split[("hash", name)] == merged[("hash", name)] == PARENT["default"][name]


def test_hyper_iterations_are_the_parent_bit_for_bit(built):
    out = _run("default")
    kp = out[("kernel", "hyper")]
    print(f"hyper: variance and scales after three ADAM(0.01) steps {kp}  sha256 {out[('hash', 'hyper')]}")
    assert kp[0] > 0 and kp[1] > 0
    assert abs(kp[1] - 3.0) > 1e-3  # the hyper steps were taken: the scale has moved off its start (ADAM: about 0.01 a step)
    if _bitwise():
        assert out[("hash", "hyper")] == PARENT["default"]["hyper"]
