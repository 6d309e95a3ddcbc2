"""The block substitution's read-ahead operands (subst_tile, agp_chol.h; DESIGN.md section 5 "round 14"): in the CAVI step's fp64
launches every T X_k' is formed in three stages of eight 16 x 16 tiles, and since round 14 each stage reads its MFMA operands ahead
of the MFMAs, one full-rate LDS read per operand -- the operands that are valid from the start (the [L21 | X22] rows of the slot and
the wave's own tile of T2) under the stage in front, across its barrier.  Same operands, same MFMA order per accumulator: every bit
of the result must be what the parent commit computed.

Five CAVI steps of Logistic SVGP (D = 4, N = 1500), one child process per setting (the levers are read once per process), at
* (m, B) = (128, 64)   one chain substitution; both k ranges (16 and 32) of the triangular stages;
* (m, B) = (136, 100)  a ragged last tile (8 valid columns) and ragged extension rows (100 = 64 + 36);
* (m, B) = (192, 64)   two chain substitutions: U is parked over a slot half that the next column's X_k reuses.
Settings: merged and split launch (AGP_CHAIN_SPLIT=0 / 1), without the prologue (AGP_STEP_PROLOGUE=0), and the two feed hooks:
AGP_DAG_TEST_FEED=1 (store_d settles every D element again) and AGP_DAG_TEST_FEED=2 (every look fails: the late path, in which
after_first is a plain barrier).  In every setting the result is compared with the CPU oracle (oracle.agp_ref) with the tolerances
of tests/test_gpu_feeder_split.py: 1e-9 on eta1 and eta2, 1e-8 on mu and Sigma.  Bit for bit (SHA-256 over mu, Sigma, eta1, eta2):
merged = split, two fresh runs, both feed hooks = the default, and all of them = PARENT below.  Under a fallback-forcing variable
(tests/_knobs.py) only the oracle comparisons apply."""
import os
import subprocess
import sys

import pytest

import _knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((128, 64), (136, 100), (192, 64))

# What the commit before round 14 (cf367b5, "Balance the chain's S = D - L L' over the SIMDs; trim the step's tail") printed for
# _RUN below on an MI355X, default settings.  Round 14 moved LDS reads and nothing else, so these hold as long as no operand, no MFMA
# order and no summation order of the step changes; a pull request that changes one of those on purpose re-pins them and says so.
PARENT = {
    128: "56e66b15ec37e4c5ceba5079bc43224e25c5a641877a65104b81111626421e64",
    136: "6e8a2bd6ef4cc7269e305925ab381aa6712b60aca18e4ee1773f047a6005d05b",
    192: "d9469f0d428456506ab4c414e51702d17241ddad689ee04b0c062889aa7f6066",
}

_RUN = r"""
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import agp_amd as AGP
from agp_amd import capi
from oracle import agp_ref as R
for m, B in ((128, 64), (136, 100), (192, 64)):
    rng = np.random.default_rng(14 + m + B)
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


def _run(key, env_extra):
    """one process per setting, the three shapes in it; shared by the tests below"""
    if key not in _cache:
        r = subprocess.run([sys.executable, "-c", _RUN, "oracle"], cwd=ROOT, env=dict(os.environ, **env_extra), capture_output=True,
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
    return _run("merged", {"AGP_CHAIN_SPLIT": "0"})


def _check_oracle(out, m):
    e_eta2, e_eta1, e_mu, e_sig = out[("err", m)]
    print(f"m = {m}: eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}  prologue steps {out[('npro', m)]}  "
          f"sha256 {out[('hash', m)]}")
    assert e_eta2 <= 1e-9 and e_eta1 <= 1e-9
    assert e_mu <= 1e-8 and e_sig <= 1e-8


def _bitwise():
    return not _knobs.forced(*_knobs._DEFAULTS)


@pytest.mark.parametrize("m,B", SHAPES)
def test_merged_launch_matches_oracle_and_the_parent_bit_for_bit(built, m, B):
    out = _merged()
    _check_oracle(out, m)
    if _bitwise():
        assert out[("hash", m)] == PARENT[m]


@pytest.mark.parametrize("m,B", SHAPES)
def test_split_launch_matches_oracle_and_is_bitwise_the_merged_launch(built, m, B):
    out = _run("split", {"AGP_CHAIN_SPLIT": "1"})
    _check_oracle(out, m)
    if _bitwise():
        assert out[("hash", m)] == _merged()[("hash", m)]


@pytest.mark.parametrize("m,B", SHAPES)
def test_two_fresh_runs_match_oracle_and_are_bitwise_equal(built, m, B):
    out = _run("again", {"AGP_CHAIN_SPLIT": "0"})
    _check_oracle(out, m)
    if _bitwise():
        assert out[("hash", m)] == _merged()[("hash", m)]


@pytest.mark.parametrize("m,B", SHAPES)
def test_without_the_prologue_matches_oracle(built, m, B):
    out = _run("noprologue", {"AGP_STEP_PROLOGUE": "0"})
    _check_oracle(out, m)
    assert out[("npro", m)] == 0


@pytest.mark.parametrize("feed", ["1", "2"])
@pytest.mark.parametrize("m,B", SHAPES)
def test_feed_hooks_match_oracle_and_are_bitwise_the_default(built, m, B, feed):
    """1: every D element settled again by store_d ; 2: every look fails -- the late path, after_first a plain barrier"""
    out = _run("feed" + feed, {"AGP_DAG_TEST_FEED": feed})
    _check_oracle(out, m)
    if _bitwise():
        default = _run("default", {})
        assert out[("hash", m)] == default[("hash", m)] == PARENT[m]
