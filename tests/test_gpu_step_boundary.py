"""The head of the C2 step launch prepared by the launch in front of it (ProArgs::pre): the first three tiles
of the pending natural-gradient step's S = kappa' diag(w) kappa are formed by the deferred fallback / row-statistics launch
(k_safe_rowstats) as partial tiles, and tile (0, 0), (1, 0), (1, 1) of the next task-graph launch add them instead of forming a
k-slice and waiting for helpers.  The summation order of those tiles changes, so the checks are against the oracle (the CAVI
step's tolerances: 1e-9 on eta, 1e-8 on mu and Sigma), bitwise against a second identical run, and with the forced-fallback hook
(AGP_DAG_TEST_ABORT=1: every launch latches a lost dependency in software, the fallback re-runs it and the partials of that launch
are marked invalid, so the next launch forms the three tiles itself)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C2's shape (m = B = 1024, D = 32, SE kernel, logistic likelihood, fp64) on a small data set; training through train_, which
# announces every next minibatch (look-ahead), so that from the second step on every launch takes the pending step in its
# prologue and, from the third on, finds the head prepared by the deferred launch in front of it
_RUN = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import agp_amd as AGP
import ctypes as C
from agp_amd import capi
from oracle import agp_ref as R
rng = np.random.default_rng(11)
N, D, m, B, iters = 4096, 32, 1024, 1024, 6
X = rng.random((N, D))
y = np.sign(np.sin(X @ rng.standard_normal(D)) + 0.1 * rng.standard_normal(N))
Z = X[rng.permutation(N)[:m]].copy()
ell = np.sqrt(D) / 4
idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
ma = AGP.SVGP(AGP.with_lengthscale(AGP.SqExponentialKernel(), ell), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z, optimiser=False)
AGP.train_(ma, X, y, iters, idx_stream=idx)
mu, Sig, e1, e2 = ma.get_state(0)
ns, npro = C.c_int64(), C.c_int64()
ma._chk(capi.lib().agp_svgp_step_counters(ma._h, C.byref(ns), C.byref(npro)))
print('PROLOGUES', npro.value)
print('HASH', hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in (mu, Sig, e1, e2))).hexdigest())
if len(sys.argv) > 1 and sys.argv[1] == 'oracle':
    mr = R.SVGP(R.Kernel("sqexponential", 1 / ell, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B)
    mr.train(X, y, iters, idx_stream=idx)
    gr = mr.latents[0]
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))
    print('ERR', rel(e2, gr.eta2), rel(e1, gr.eta1), rel(mu, gr.mu), rel(Sig, gr.Sigma))
"""


def _run(env_extra, *argv):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _RUN, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        k, _, v = line.partition(" ")
        if k in ("PROLOGUES", "HASH", "ERR"):
            out[k] = v
    return out


def _check_oracle(out):
    e_eta2, e_eta1, e_mu, e_sig = (float(v) for v in out["ERR"].split())
    print(f"eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}  prologue steps {out['PROLOGUES']}")
    assert int(out["PROLOGUES"]) >= 3  # the pending step rode on the step launches (so the prepared head was in use)
    assert e_eta2 <= 1e-9 and e_eta1 <= 1e-9
    assert e_mu <= 1e-8 and e_sig <= 1e-8


def test_c2_shape_with_prepared_head_matches_oracle(built):
    _check_oracle(_run({}, "oracle"))


def test_c2_shape_with_prepared_head_is_bitwise_reproducible(built):
    a, b = _run({}), _run({})
    assert a["HASH"] == b["HASH"]


@pytest.mark.parametrize("split", ["0", "1"])
def test_forced_fallback_with_prepared_head_matches_oracle(built, split):
    """every launch latches -1 (AGP_DAG_TEST_ABORT=1): the deferred launch re-runs the factorisation and the rows, marks its
    partials invalid, and the next launch's first three tiles form their products themselves -- merged and split launches"""
    _check_oracle(_run({"AGP_DAG_TEST_ABORT": "1", "AGP_CHAIN_SPLIT": split}, "oracle"))
