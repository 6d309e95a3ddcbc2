"""The CAVI step's task-graph launches store no diagonal factors (dag_store_dg, agp_chol.h): Dg is valid only
while Xa is, and every reader of Dg -- the log-determinant sums of the ELBO's Gaussian KL and of online_snapshot -- sits behind
materialize(), which factors again with the inverse riding along whenever a step launch came last.

Handle 1 takes CAVI steps; a fresh handle 2, which has never run a step launch, is brought to the same natural parameters through
set_state.  Whatever is read from the two must then be bit for bit the same: the ELBO, (mu, Sigma) of get_state and the three
results of online_snapshot (D_a^-1, eta1 and the constant with the log-determinant).  Read three times: after five steps, after one
more step (the handle has its inverse, the step waits as a pending one and is taken by flush()), and after two more (a step launch
again, then the pending step).  Both types, two and three block columns, a whole and a ragged batch, merged and split launch (forced
the way tests/test_gpu_block_substitution.py forces them)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(t, m, B) for t in ("f64", "f32") for m in (128, 192) for B in (64, 200)]
PHASES = ("5 steps", "+1 step", "+2 steps")

_RUN = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import torch
import agp_amd as AGP
from agp_amd import capi

def model(Z, B, T):
    return AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                    optimiser=False, T=T)

def read(mo, Xe, ye):
    mu, Sig, e1, e2 = mo.get_state(0)
    elbo = AGP.ELBO(mo, Xe, ye, rho=1.0)
    iD = torch.empty(mo.m, mo.m, dtype=mo.tdtype, device=mo._dev())
    s1 = torch.empty(mo.m, dtype=mo.tdtype, device=mo._dev())
    pl = C.c_double()
    mo._chk(capi.lib().agp_svgp_online_snapshot(mo._h, 0, C.c_void_p(iD.data_ptr()), mo.m, C.c_void_p(s1.data_ptr()), C.byref(pl)))
    return dict(mu=mu, Sigma=Sig, eta1=e1, eta2=e2, elbo=np.float64(elbo), invDa=iD.cpu().numpy(), snap_eta1=s1.cpu().numpy(),
                logdet_term=np.float64(pl.value))

for tname, T in (("f64", np.float64), ("f32", np.float32)):
    for m in (128, 192):
        for B in (64, 200):
            rng = np.random.default_rng(100 + m + B)
            N, D, iters = 1500, 4, 8
            X = rng.random((N, D)); f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
            y = np.sign(f + 0.3 * rng.standard_normal(N))
            Z = X[rng.permutation(N)[:m]].copy()
            idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
            m1, m2 = model(Z, B, T), model(Z, B, T)
            m2._ensure_handle(B)
            done = 0
            for phase, more in enumerate((5, 1, 2)):
                AGP.train_(m1, X, y, more, idx_stream=idx[done:done + more], **({"state": True} if done else {}))
                done += more
                a = read(m1, X[:B], y[:B])
                m2.set_state(0, a["eta1"], a["eta2"])
                b = read(m2, X[:B], y[:B])
                bad = [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
                fin = all(np.all(np.isfinite(np.asarray(v))) for v in a.values())
                print("CASE", tname, m, B, phase, "finite" if fin else "nonfinite", ",".join(bad) if bad else "equal", flush=True)
            ns, npro = C.c_int64(), C.c_int64()
            m1._chk(capi.lib().agp_svgp_step_counters(m1._h, C.byref(ns), C.byref(npro)))
            print("STEPS", tname, m, B, ns.value, npro.value, flush=True)
"""

_cache = {}


def _run(split):
    if split not in _cache:
        r = subprocess.run([sys.executable, "-c", _RUN], cwd=ROOT, env=dict(os.environ, AGP_CHAIN_SPLIT=split), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w and w[0] == "CASE":
                out[(w[1], int(w[2]), int(w[3]), int(w[4]))] = (w[5], w[6])
            elif w and w[0] == "STEPS":
                out[(w[1], int(w[2]), int(w[3]), "steps")] = (int(w[4]), int(w[5]))
        _cache[split] = out
    return _cache[split]


@pytest.mark.parametrize("split", ["0", "1"], ids=["merged", "split"])
@pytest.mark.parametrize("tname,m,B", CASES)
def test_handle_after_step_launches_reads_like_a_fresh_handle(built, tname, m, B, split):
    out = _run(split)
    nsteps, npro = out[(tname, m, B, "steps")]
    print(f"{tname} m={m} B={B} split={split}: {nsteps} steps, {npro} with the pending step as prologue")
    assert nsteps == 8 and npro >= 3  # the step launches ran with the pending step in front (DagStepPro), not only the plain ones
    for phase, what in enumerate(PHASES):
        fin, diff = out[(tname, m, B, phase)]
        print(f"  after {what}: {fin}, {diff}")
        assert fin == "finite"
        assert diff == "equal", f"after {what}: handle 1 and the fresh handle differ in {diff}"
