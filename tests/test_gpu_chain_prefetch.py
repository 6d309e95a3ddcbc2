"""The chain workgroup's side job (ChainPrefetch in csrc/agp_chol.h) brings the two feeder tiles of the next block column into LDS
while a tile elimination runs.  In fp64 launches the first tile, T = (k+1, k), is consumed three rounds after its loads were issued
and the second, D = (k+1, k+1), behind the elimination, in front of its first reader.  Three paths lead to the same data:

* prefetched          the look in round 3 saw both feeders' flags, T came whole, D is stored from registers behind the substitution;
* settled             ... and a D element that still reads as the sentinel is re-loaded in place (AGP_DAG_TEST_FEED=1 sends every
                      element that way);
* late                the look failed or T held a sentinel: both tiles come through the blocking fetch (AGP_DAG_TEST_FEED=2 makes
                      every look fail).

All of them re-load valid data, so every result must be the same bits whichever path ran, merged launch or chain kernel + tile kernel
(AGP_CHAIN_SPLIT).  The library reads its environment once per process: every setting runs in a child process of its own, all of
them started together, each computing every case once and printing SHA-256 hashes; the tests compare the reports.

Cases: SVGP, 5 CAVI steps, m = 128 / 192 / 320 (nt = 2: one prefetch, whose D is the last diagonal tile; nt = 3: the first column
with the Dg and the L copies in front of a prefetch; nt = 5), B = 64 and 200 (ragged), both types; agp_potrf_jitter (chain launches
that store L and the real Dg) at n = 64 (no prefetch), 128, 130, 200, both types; one batched launch of three latents."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SVGP_CASES = [(m, B, tn) for tn in ("f64", "f32") for m in (128, 192, 320) for B in (64, 200)]
POTRF_CASES = [(n, tn) for tn in ("f64", "f32") for n in (64, 128, 130, 200)]
FEEDS = ("", "1", "2")
SETTINGS = [(feed, split) for split in ("0", "1") for feed in FEEDS]  # (AGP_DAG_TEST_FEED, AGP_CHAIN_SPLIT)

_CHILD = r"""
import ctypes as C, hashlib, json, sys
import numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as g; g.build()
import torch
import agp_amd as AGP
from agp_amd import capi

sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}

def data(seed, N, D, m, B, iters):
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    f = np.sin(4 * X[:, 0]) + X[:, 1] - 0.8
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [rng.choice(N, B, replace=False) for _ in range(iters)]
    return rng, X, f, Z, idx

for tn, T in (("f64", np.float64), ("f32", np.float32)):
    for m in (128, 192, 320):
        for B in (64, 200):
            rng, X, f, Z, idx = data(1000 * m + B, 2000, 4, m, B, 5)
            y = np.sign(f + 0.3 * rng.standard_normal(2000))
            model = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticLikelihood(), AGP.AnalyticSVI(B), Z,
                             optimiser=False, T=T)
            AGP.train_(model, X, y, 5, idx_stream=idx)
            mu, Sig, _, _ = model.get_state(0)
            out[f"svgp_{tn}_m{m}_B{B}"] = {"mu": sha(mu), "Sigma": sha(Sig), "elbo": float(AGP.ELBO(model, X[:B], y[:B])).hex()}

# three latents in one batched launch, twice
rng, X, f, Z, idx = data(77, 1500, 4, 128, 64, 5)
y3 = 1 + np.digitize(f, np.quantile(f, [0.33, 0.66]))
for run in (0, 1):
    model = AGP.SVGP(AGP.SqExponentialKernel() @ AGP.ScaleTransform(3.0), AGP.LogisticSoftMaxLikelihood(3), AGP.AnalyticSVI(64), Z,
                     optimiser=False)
    AGP.train_(model, X, y3, 5, idx_stream=idx)
    h = hashlib.sha256()
    for l in range(3):
        for a in model.get_state(l):
            h.update(np.ascontiguousarray(a).tobytes())
    out[f"batched_run{run}"] = h.hexdigest()

L = capi.lib()
for tn, dt in (("f64", 0), ("f32", 1)):
    for n in (64, 128, 130, 200):
        G = np.random.default_rng(n).standard_normal((n, n + 8))
        A = G @ G.T / n + 0.5 * np.eye(n)
        ctx = C.c_void_p()
        assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
        ad = torch.tensor(A, dtype=torch.float32 if dt else torch.float64, device="cuda").contiguous()
        given = ad.cpu().numpy().astype(np.float64)
        info = C.c_int32(-7)
        st = L.agp_potrf_jitter(ctx, dt, C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        torch.cuda.synchronize()
        L.agp_ctx_destroy(ctx)
        assert st == 0 and info.value == 0, (st, info.value, n, tn)
        Lf = np.tril(ad.cpu().numpy().astype(np.float64))
        ref = np.linalg.cholesky(given)
        out[f"potrf_{tn}_n{n}"] = {
            "L": sha(ad.cpu().numpy()),
            "res": float(np.abs(Lf @ Lf.T - given).max() / np.abs(given).max()),
            # sum_i log L_ii: the diagonal tiles come from Dg (k_publish_diag), which is what the ELBO's log det reads
            "half_logdet": float(np.sum(np.log(np.diag(Lf)))), "half_logdet_ref": float(np.sum(np.log(np.diag(ref)))),
            "amax": float(np.abs(given).max()), "lmin": float(np.linalg.eigvalsh(given)[0])}
print("REPORT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def reports(built):
    """{(feed, split): report} -- six child processes side by side, every case computed once per setting"""
    procs = {}
    for feed, split in SETTINGS:
        env = dict(os.environ, AGP_CHAIN_SPLIT=split)
        env.pop("AGP_DAG_TEST_FEED", None)
        if feed:
            env["AGP_DAG_TEST_FEED"] = feed
        procs[(feed, split)] = subprocess.Popen([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE, text=True)
    res = {}
    for key, p in procs.items():
        try:
            so, se = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, (key, so[-2000:], se[-2000:])
        res[key] = json.loads([l for l in so.splitlines() if l.startswith("REPORT ")][0][len("REPORT "):])
    return res


@pytest.mark.parametrize("m,B,tn", SVGP_CASES)
def test_svgp_bits_equal_on_every_feed_path_merged_and_split(reports, m, B, tn):
    """mu, Sigma (get_state) and the ELBO after 5 CAVI steps: the same bits for AGP_DAG_TEST_FEED unset / 1 / 2, one kernel or two"""
    key = f"svgp_{tn}_m{m}_B{B}"
    base = reports[("", "0")][key]
    print(key, base)
    for s in SETTINGS:
        assert reports[s][key] == base, (s, reports[s][key], base)


@pytest.mark.parametrize("n,tn", POTRF_CASES)
def test_potrf_factor_bits_equal_on_every_feed_path(reports, n, tn):
    """L of agp_potrf_jitter: the same bits on the three paths; ||L L' - A|| / ||A|| (max norm) <= 4 n u as in
    tests/test_gpu_tile_rounds.py; and sum_i log L_ii, read from the published Dg tiles, against numpy's float64 factor of the same
    matrix.  Bound for the latter: L L' = A + E with |E| <= 4 n u |A|max elementwise (the residual bound just asserted), and
    |log det(A + E) - log det A| <= n ||A^-1||_2 ||E||_2 (1 + o(1)) <= n (1 / lambda_min) n 4 n u |A|max; half of it for the factor's
    diagonal, doubled for the second-order term and numpy's own error: 4 n^3 u |A|max / lambda_min."""
    key = f"potrf_{tn}_n{n}"
    base = reports[("", "0")][key]
    u = 2.0 ** -24 if tn == "f32" else 2.0 ** -53
    bound = 4 * n * u
    ld_bound = 4 * n ** 3 * u * base["amax"] / base["lmin"]
    ld_err = abs(base["half_logdet"] - base["half_logdet_ref"])
    print(f"{key}: residual {base['res']:.3e} (bound {bound:.3e})  sum log L_ii {base['half_logdet']:.12g} vs numpy "
          f"{base['half_logdet_ref']:.12g}: {ld_err:.3e} (bound {ld_bound:.3e})")
    assert base["res"] <= bound
    assert ld_err <= ld_bound
    for s in SETTINGS:
        assert reports[s][key]["L"] == base["L"], s
        assert reports[s][key]["half_logdet"] == base["half_logdet"], s


def test_batched_launch_bits_equal_between_runs_and_feed_paths(reports):
    """three latents (LogisticSoftMax, m = 128, B = 64) in one interleaved launch: eta, mu, Sigma of all of them"""
    base = reports[("", "0")]["batched_run0"]
    for s in SETTINGS:
        assert reports[s]["batched_run0"] == base, s
        assert reports[s]["batched_run1"] == base, s
