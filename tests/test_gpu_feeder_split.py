"""The k-split of the step launch's prologue re-fitted to the chain's pace (pro_ks_table, agp_chol_host.h): from
four block columns on the near-diagonal tiles of a block column take a finer split than the rest of it, so that the diagonal feeder
(c, c) is parked when the chain's side job looks for it.  m = 448 is seven block columns (columns 3 and 5 have near tiles), and
B = 1024 / 1000 gives nq = 16 chunks -- the smallest at which the changed entries are reached -- the second with a partial last
chunk.  The split moves the order in which the partial tiles of S = kappa' diag(w) kappa are summed, so the state is checked against
the CPU oracle with the tolerances of tests/test_gpu_step_boundary.py (1e-9 on eta, 1e-8 on mu and Sigma); merged against split
launch and two fresh runs bit for bit; and with AGP_STEP_PROLOGUE=0 (no prologue, no table) within the same tolerances."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1024, 1000)

_RUN = r"""
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import agp_amd as AGP
from agp_amd import capi
from oracle import agp_ref as R
for B in (1024, 1000):
    rng = np.random.default_rng(31 + B)
    N, D, m, iters = 3000, 4, 448, 3
    X = rng.random((N, D)); f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
    y = np.sign(f + 0.3 * rng.standard_normal(N))
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    ma = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
    AGP.train_(ma, X, y, iters, idx_stream=idx)
    mu, Sig, e1, e2 = ma.get_state(0)
    ns, npro = C.c_int64(), C.c_int64()
    ma._chk(capi.lib().agp_svgp_step_counters(ma._h, C.byref(ns), C.byref(npro)))
    print('RUN', B, npro.value, hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in (mu, Sig, e1, e2))).hexdigest())
    if len(sys.argv) > 1 and sys.argv[1] == 'oracle':
        mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
        mr.train(X, y, iters, idx_stream=idx)
        gr = mr.latents[0]
        rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))
        print('ERR', B, rel(e2, gr.eta2), rel(e1, gr.eta1), rel(mu, gr.mu), rel(Sig, gr.Sigma))
"""

_cache = {}


def _run(key, env_extra, *argv):
    """one process per setting (the levers are read once per process), both batch sizes in it; shared by the tests below"""
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


def _check_oracle(out, B):
    e_eta2, e_eta1, e_mu, e_sig = out[("err", B)]
    print(f"B = {B}: eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}  prologue steps {out[('npro', B)]}")
    assert e_eta2 <= 1e-9 and e_eta1 <= 1e-9
    assert e_mu <= 1e-8 and e_sig <= 1e-8


@pytest.mark.parametrize("B", BATCHES)
def test_seven_block_columns_match_oracle(built, B):
    out = _merged()
    _check_oracle(out, B)
    assert out[("npro", B)] >= 2  # steps 2 and 3 took the pending step as their prologue: the table was in use


@pytest.mark.parametrize("B", BATCHES)
def test_split_launch_is_bitwise_the_merged_launch(built, B):
    assert _run("split", {"AGP_CHAIN_SPLIT": "1"})[("hash", B)] == _merged()[("hash", B)]


@pytest.mark.parametrize("B", BATCHES)
def test_two_fresh_runs_are_bitwise_equal(built, B):
    assert _run("again", {"AGP_CHAIN_SPLIT": "0"})[("hash", B)] == _merged()[("hash", B)]


@pytest.mark.parametrize("B", BATCHES)
def test_without_the_prologue_matches_oracle(built, B):
    out = _run("noprologue", {"AGP_STEP_PROLOGUE": "0"}, "oracle")
    _check_oracle(out, B)
    assert out[("npro", B)] == 0
