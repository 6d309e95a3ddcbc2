"""The last block column of a CAVI step launch stores only what somebody reads (agp_chol.h, `tail_row`; DESIGN.md section 5 "round
13"): the kappa rows' tiles (R, nt - 1) of an fp64 step launch with the epilogue keep their W in its real home but neither fill their
hand-over slot nor raise their flag -- no tile of the launch looks at either.  Whatever is read from the handle afterwards must not
notice.

Handle 1 takes CAVI steps; a fresh handle 2, which has never run a step launch, is brought to the same natural parameters through
set_state (the scheme of tests/test_gpu_step_stores_no_dg.py).  The ELBO, (mu, Sigma) of get_state, predict_f (mean and variance) and
the three results of online_snapshot must then be bit for bit the same.  Read three times: after five steps, after one more step
(it waits as a pending step and is taken by flush()), and after two more.  Both types, two and three block columns, B = 64 and a
ragged B = 100, merged and split launch.  With AGP_DAG_TEST_ABORT=1 every step launch hands its step to the in-stream fallback, which
factors again and rewrites W (by other kernels, in another order of summation than the factorisation behind set_state: no bit
equality there): the state after the eight steps is compared with the CPU oracle, with the tolerances of
tests/test_gpu_step_boundary.py for fp64 (1e-9 on eta, 1e-8 on mu and Sigma) and, for fp32, the 5e-3 and the oracle jitter 1e-3 of
the fp32 case of tests/test_gpu_round3.py (test_pending_step_is_invisible_through_the_abi)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(t, m, B) for t in ("f64", "f32") for m in (128, 192) for B in (64, 100)]
PHASES = ("5 steps", "+1 step", "+2 steps")

_RUN = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import torch
import agp_amd as AGP
from agp_amd import capi
from oracle import agp_ref as R

def model(Z, B, T):
    return AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                    optimiser=False, T=T)

def read(mo, Xe, ye):
    mu, Sig, e1, e2 = mo.get_state(0)
    elbo = AGP.ELBO(mo, Xe, ye, rho=1.0)
    pm, pv = AGP.predict_f(mo, Xe, cov=True)
    iD = torch.empty(mo.m, mo.m, dtype=mo.tdtype, device=mo._dev())
    s1 = torch.empty(mo.m, dtype=mo.tdtype, device=mo._dev())
    pl = C.c_double()
    mo._chk(capi.lib().agp_svgp_online_snapshot(mo._h, 0, C.c_void_p(iD.data_ptr()), mo.m, C.c_void_p(s1.data_ptr()), C.byref(pl)))
    return dict(mu=mu, Sigma=Sig, eta1=e1, eta2=e2, elbo=np.float64(elbo), pred_mean=np.asarray(pm), pred_var=np.asarray(pv),
                invDa=iD.cpu().numpy(), snap_eta1=s1.cpu().numpy(), logdet_term=np.float64(pl.value))

oracle = len(sys.argv) > 1 and sys.argv[1] == 'oracle'
for tname, T in (("f64", np.float64), ("f32", np.float32)):
    for m in (128, 192):
        for B in (64, 100):
            rng = np.random.default_rng(300 + m + B)
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
            if oracle:
                mr = R.SVGP(R.Kernel("sqexponential", 3.0, 1.0), R.LogisticLikelihood(), Z, stochastic=True, batchsize=B,
                            jitter=1e-4 if T == np.float64 else 1e-3)
                mr.train(X, y, iters, idx_stream=idx)
                gr = mr.latents[0]
                rel = lambda p, q: float(np.max(np.abs(np.asarray(p, dtype=np.float64) - q)) / np.max(np.abs(q)))
                print("ERR", tname, m, B, rel(a["eta2"], gr.eta2), rel(a["eta1"], gr.eta1), rel(a["mu"], gr.mu), rel(a["Sigma"], gr.Sigma),
                      flush=True)
"""

_cache = {}


def _run(key, env_extra, *argv):
    if key not in _cache:
        r = subprocess.run([sys.executable, "-c", _RUN, *argv], cwd=ROOT, env=dict(os.environ, **env_extra), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w and w[0] == "CASE":
                out[(w[1], int(w[2]), int(w[3]), int(w[4]))] = (w[5], w[6])
            elif w and w[0] == "STEPS":
                out[(w[1], int(w[2]), int(w[3]), "steps")] = (int(w[4]), int(w[5]))
            elif w and w[0] == "ERR":
                out[(w[1], int(w[2]), int(w[3]), "err")] = tuple(float(v) for v in w[4:8])
        _cache[key] = out
    return _cache[key]


def _check_equal(out, tname, m, B):
    for phase, what in enumerate(PHASES):
        fin, diff = out[(tname, m, B, phase)]
        print(f"  after {what}: {fin}, {diff}")
        assert fin == "finite"
        assert diff == "equal", f"after {what}: handle 1 and the fresh handle differ in {diff}"


@pytest.mark.parametrize("split", ["0", "1"], ids=["merged", "split"])
@pytest.mark.parametrize("tname,m,B", CASES)
def test_handle_after_step_launches_reads_like_a_fresh_handle(built, tname, m, B, split):
    out = _run("split" + split, {"AGP_CHAIN_SPLIT": split})
    nsteps, npro = out[(tname, m, B, "steps")]
    print(f"{tname} m={m} B={B} split={split}: {nsteps} steps, {npro} with the pending step as prologue")
    assert nsteps == 8
    _check_equal(out, tname, m, B)


@pytest.mark.parametrize("tname,m,B", CASES)
def test_step_handed_to_the_in_stream_fallback_matches_oracle(built, tname, m, B):
    out = _run("abort", {"AGP_DAG_TEST_ABORT": "1"}, "oracle")
    assert out[(tname, m, B, "steps")][0] == 8
    e_eta2, e_eta1, e_mu, e_sig = out[(tname, m, B, "err")]
    print(f"{tname} m={m} B={B}: eta2 {e_eta2:.2e}  eta1 {e_eta1:.2e}  mu {e_mu:.2e}  Sigma {e_sig:.2e}")
    te, ts = (1e-9, 1e-8) if tname == "f64" else (5e-3, 5e-3)
    assert e_eta2 <= te and e_eta1 <= te
    assert e_mu <= ts and e_sig <= ts
