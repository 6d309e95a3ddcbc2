"""The chain's S = D - L L' in one balanced pass (dag_chain_balance, mma_tile16_chain, elim_block32<.., JOIN>; agp_chol.h, DESIGN.md
section 5 "round 13"): in fp64 chains the two accumulation chains of the result tiles (0, 0) and (1, 0) of S run on two waves each, the
even one lands in the tile, the odd one in the rounds' scratch, and the next elimination's first load adds them -- through the
mirrored index (lo, hi) for the elements above the diagonal of tile (0, 0).  The split tiles exist from the second block column on.

* agp_potrf_jitter (jitter 0, fp64) at n = 128 (two whole tiles), 136 (a ragged second tile: 8 valid columns, all of them inside
  the split tiles) and 320 (five block columns): ||L L' - A|| / ||A|| (max norm) <= 4 n u as in tests/test_gpu_tile_rounds.py, and
  against numpy.linalg.cholesky of the same matrix within 64 n u ||L|| -- these matrices have condition numbers below 12, and the
  factor's forward error is bounded by a small multiple of cond(A) n u (Higham, Accuracy and Stability, theorem 10.8).
* a matrix that is not positive definite, whose first bad pivot lies in columns 64 .. 79: the columns of the split tiles of block
  column 1.  The diagonal entry is lowered so that the pivot, D - L L' at that entry, is -1e-6 times what it was; had a half of the
  accumulation been lost the pivot would be far from zero on one side or the other.  The CPU oracle is the first leading minor
  whose Cholesky factorisation fails.
* SVGP after 5 CAVI steps at (m, B) = (128, 64) and (448, 100) against the CPU oracle with the tolerances of
  tests/test_gpu_feeder_split.py (1e-9 on eta, 1e-8 on mu and Sigma); merged against split launch and two fresh runs bit for bit;
  and with AGP_STEP_PROLOGUE=0.  Under a fallback-forcing variable (tests/_knobs.py) only the oracle comparisons apply."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 64), (448, 100))
_SPD = {}


def _spd(n):
    """A = G G' / n + I / 2 with G n x (n + 8), seeded by n; computed once per n and never modified (callers copy)"""
    if n not in _SPD:
        G = np.random.default_rng(n).standard_normal((n, n + 8))
        A = G @ G.T / n + 0.5 * np.eye(n)
        A.setflags(write=False)
        _SPD[n] = A
    return _SPD[n]


@pytest.fixture(scope="module")
def mods(built):
    import torch

    assert torch.cuda.is_available()
    from agp_amd import capi

    return capi, torch


def _potrf(mods, A):
    capi, torch = mods
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        n = A.shape[0]
        ad = torch.tensor(A, dtype=torch.float64, device="cuda").contiguous()
        info = C.c_int32(-7)
        st = L.agp_potrf_jitter(ctx, 0, C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        torch.cuda.synchronize()
        return st, info.value, ad.cpu().numpy()
    finally:
        L.agp_ctx_destroy(ctx)


@pytest.mark.parametrize("n", [128, 136, 320])
def test_factor_against_the_cpu_oracle(mods, n):
    A = _spd(n)
    st, info, out = _potrf(mods, A)
    assert st == 0 and info == 0, (st, info)
    Lf = np.tril(out)
    u = 2.0 ** -53
    res = np.abs(Lf @ Lf.T - A).max() / np.abs(A).max()
    Lr = np.linalg.cholesky(A)
    fwd = np.abs(Lf - Lr).max() / np.abs(Lr).max()
    print(f"n = {n}: residual {res:.3e} (bound {4 * n * u:.3e}), against the oracle's factor {fwd:.3e} (bound {64 * n * u:.3e})")
    assert res <= 4 * n * u, (res, 4 * n * u)
    assert fwd <= 64 * n * u, (fwd, 64 * n * u)


def _oracle_first_bad(A, lo, hi):
    """1-based order of the first leading minor of A in (lo, hi] whose Cholesky factorisation fails (0: none)"""
    for k in range(lo + 1, hi + 1):
        try:
            np.linalg.cholesky(A[:k, :k])
        except np.linalg.LinAlgError:
            return k
    return 0


@pytest.mark.parametrize("n,bad", [(128, 64), (128, 71), (136, 79), (320, 72)])
def test_first_bad_pivot_inside_the_split_tiles(mods, n, bad):
    A = _spd(n).copy()
    Lr = np.linalg.cholesky(A[:bad + 1, :bad + 1])
    pivot = Lr[bad, bad] ** 2  # = A[bad, bad] - |L[bad, :bad]|^2, the entry of D - L L' that the elimination meets
    A[bad, bad] -= pivot * (1 + 1e-6)
    want = _oracle_first_bad(A, 0, n)
    assert want == bad + 1  # (the oracle itself: the leading block of order `bad` is untouched)
    st, info, _ = _potrf(mods, A)
    print(f"n = {n}, bad column {bad}: pivot was {pivot:.3e}, status {st}, info {info}, oracle {want}")
    assert st == 2 and info == want, (st, info, want)


_RUN = r"""
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import agp_amd as AGP
from agp_amd import capi
from oracle import agp_ref as R
for m, B in ((128, 64), (448, 100)):
    rng = np.random.default_rng(13 + m + B)
    N, D, iters = 1500, 4, 5
    X = rng.random((N, D)); f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
    y = np.sign(f + 0.3 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    mu, Sig, e1, e2 = ma.get_state(0)
    ns, npro = C.c_int64(), C.c_int64()
    ma._chk(capi.lib().agp_svgp_step_counters(ma._h, C.byref(ns), C.byref(npro)))
    print('RUN', m, npro.value, hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in (mu, Sig, e1, e2))).hexdigest())
    if len(sys.argv) > 1 and sys.argv[1] == 'oracle':
        mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
        mr.train(X, y, iters, idx_stream=idx)
        gr = mr.latents[0]
        rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))
        print('ERR', m, rel(e2, gr.eta2), rel(e1, gr.eta1), rel(mu, gr.mu), rel(Sig, gr.Sigma))
"""

_cache = {}


def _run(key, env_extra, *argv):
    """one process per setting (the levers are read once per process), both shapes in it; shared by the tests below"""
    if key not in _cache:
        r = subprocess.run([sys.executable, "-c", _RUN, *argv], cwd=ROOT, env=dict(os.environ, **env_extra), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w and w[0] == "RUN":
                out[("npro", int(w[1]))], out[("hash", int(w[1]))] = int(w[2]), w[3]
            elif w and w[0] == "ERR":
                out[("err", int(w[1]))] = tuple(float(v) for v in w[2:6])
        _cache[key] = out
    return _cache[key]


def _merged():
    return _run("merged", {"AGP_CHAIN_SPLIT": "0"}, "oracle")


def _check_oracle(out, m):
    e_eta2, e_eta1, e_mu, e_sig = out[("err", m)]
    print(f"m = {m}: eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}  prologue steps {out[('npro', m)]}")
    assert e_eta2 <= 1e-9 and e_eta1 <= 1e-9
    assert e_mu <= 1e-8 and e_sig <= 1e-8


@pytest.mark.parametrize("m,B", SHAPES)
def test_five_steps_match_oracle(built, m, B):
    _check_oracle(_merged(), m)


@pytest.mark.parametrize("m,B", SHAPES)
def test_split_launch_matches_oracle_and_is_bitwise_the_merged_launch(built, m, B):
    out = _run("split", {"AGP_CHAIN_SPLIT": "1"}, "oracle")
    _check_oracle(out, m)
    if not _knobs.forced(*_knobs._DEFAULTS):
        assert out[("hash", m)] == _merged()[("hash", m)]


@pytest.mark.parametrize("m,B", SHAPES)
def test_two_fresh_runs_match_oracle_and_are_bitwise_equal(built, m, B):
    out = _run("again", {"AGP_CHAIN_SPLIT": "0"}, "oracle")
    _check_oracle(out, m)
    if not _knobs.forced(*_knobs._DEFAULTS):
        assert out[("hash", m)] == _merged()[("hash", m)]


@pytest.mark.parametrize("m,B", SHAPES)
def test_without_the_prologue_matches_oracle(built, m, B):
    out = _run("noprologue", {"AGP_STEP_PROLOGUE": "0"}, "oracle")
    _check_oracle(out, m)
    assert out[("npro", m)] == 0
