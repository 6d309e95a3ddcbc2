"""The conditions tests/test_gpu_hyper_edges.py rests on, checked with no device in the loop, on every case of tests/_hyper_cases.py.

Where tests/_torch_elbo.py restates the objective (Logistic, Gaussian, StudentT), the oracle's hand-derived R.hyper_gradient (pinned
by finite differences in tests/test_oracle_kat.py) and torch.autograd of the restatement, both at the oracle's own state as in
tests/test_oracle_autograd.py, agree to 1e-9 -- dvariance relative to max(1, |.|), dscale and dZ relative to the vector's largest
entry.  A case that misses this is too ill-conditioned to pin the device at 1e-7: its scale in the recipe changes, not the bound.

On every case and every latent, the reference gradient
* leaves no column of dZ below 0.05 of dZ's largest entry: a max-norm comparison at 1e-7 then still pins every input dimension to
  2e-6 of its own size, so a wrong dimension cannot hide behind a larger one;
* is not trivially small: |dvariance| or max |dscale| above 1e-3 (otherwise another seed in the table)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import agp_ref as R  # noqa: E402

import _hyper_cases as HC  # noqa: E402
import _torch_elbo as TE  # noqa: E402


@pytest.mark.parametrize("c", HC.CASES, ids=HC.case_id)
def test_references_agree_and_no_dimension_hides(c):
    M, xb, yb, rho, grads = HC.oracle_run(c, R)
    for k, g in enumerate(grads):
        dz = g["dZ"]
        assert g["dscale"].shape == (c["D"],) and dz.shape == (c["m"], c["D"])
        cols = np.max(np.abs(dz), axis=0) / np.max(np.abs(dz))
        print(f"{HC.case_id(c)} latent {k}: smallest dZ column {cols.min():.3f} of the largest; |dvariance| {abs(g['dvariance']):.2e} "
              f"max |dscale| {np.max(np.abs(g['dscale'])):.2e}; cond(K) {np.linalg.cond(M.latents[k].K):.1e}")
        assert cols.min() >= 0.05
        assert abs(g["dvariance"]) > 1e-3 or np.max(np.abs(g["dscale"])) > 1e-3
    if c["lik"] not in HC.RESTATED:
        return
    gp, g = M.latents[0], grads[0]
    local = {} if c["lik"] == "gaussian" else {"theta": M.local_vars["theta"]}
    dv, ds, dz, _ = TE.autograd_hypergrad(c["kind"], HC.restated_lik(c), xb, np.asarray(yb, dtype=np.float64), gp.Z, gp.kernel.scale,
                                          gp.kernel.sigma2, gp.mu, gp.Sigma, gp.mu0, local, rho, M.jitter, c["mode"])
    ev, es, ez = HC.errors((g["dvariance"], g["dscale"], g["dZ"]), (dv, ds, dz))
    print(f"{HC.case_id(c)}: oracle vs autograd dvariance {ev:.1e} dscale {es:.1e} dZ {ez:.1e}")
    assert ev < 1e-9 and es < 1e-9 and ez < 1e-9


def test_the_table_reaches_every_branch():
    """one hyper-gradient case at least in each regime the device code tells apart"""
    cs = HC.CASES
    assert any(c["D"] <= 32 for c in cs) and any(32 < c["D"] <= 64 for c in cs)
    assert {1, 31, 32, 33, 64} <= {c["D"] for c in cs}
    assert any(c["m"] % 64 for c in cs) and any(c["B"] % 64 for c in cs)
    assert any(c["m"] % 64 == 0 and c["m"] >= 128 and c["B"] % 64 == 0 for c in cs)  # the fused G_K
    assert {"ard", "scale", "none"} <= {c["transform"] for c in cs if c["D"] > 32}
    assert {"logistic", "gaussian", "studentt", "bayesiansvm", "heteroscedastic", "logisticsoftmax"} <= {c["lik"] for c in cs}
    assert all(c["D"] > 32 and (c["m"] % 64 or c["B"] % 64) for c in HC.F32_CASES)
    assert {1, 32, 33, 64} <= {D for D, _, _, _ in HC.VGP_CASES} and {65, 130} <= {N for _, N, _, _ in HC.VGP_CASES}
    assert len({HC.case_id(c) for c in cs + HC.F32_CASES}) == len(cs) + len(HC.F32_CASES)
