"""The class-count cases without a GPU (tests/_multiclass_cases.py): what every case claims to reach is recomputed from the
constants in the headers under csrc/, so a changed constant fails here and forces a new choice of K; every class occurs in every
minibatch; the oracle's trajectory of every case is finite.  The margin condition of the Monte-Carlo trajectory cases is asserted by
tests/test_mcvi_host.py (test_margin_condition_on_every_parity_input) on the cases this work added to tests/_mcvi_cases.py."""
import os
import re

import numpy as np
import pytest

import _mcvi_cases as CS
import _multiclass_cases as MK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgaussianprocesses.jl_amd", "csrc")
NAMES = ("CHOL_MAXB", "DAG_MAX_NB", "DAG_MAX_NT", "DAG_MAX_COLUMN_TILES", "ROWSTATS_MAXB", "SYRK_MAXB", "LSM_FUSED_MAXL", "MO_MAXT",
         "MC_KMAX", "MC_TILE")


@pytest.fixture(scope="module")
def consts():
    text = "\n".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")))
    out = {}
    for n in NAMES:
        found = set(re.findall(r"constexpr\s+(?:int|int64_t)\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + n + r"\s*=\s*(\d+)", text))
        assert len(found) == 1, (n, found)
        out[n] = int(found.pop())
    return out


def _rup(n, t=MK.TILE):
    return (n + t - 1) // t * t


def _pow2_at_least(K, lo):
    p = lo
    while p < K:
        p <<= 1
    return p


def _chunks(n, chunk):
    return tuple(min(chunk, n - a) for a in range(0, n, chunk))


def _dag_nb(c, m, B):
    """step_local: the largest q <= DAG_MAX_NB with q (nt + ne + 1) <= DAG_MAX_COLUMN_TILES and nt <= DAG_MAX_NT (chol_use_dag)"""
    nt, ne = _rup(m) // MK.TILE, _rup(B) // MK.TILE + 1
    for q in range(c["DAG_MAX_NB"], 0, -1):
        if q * (nt + ne + 1) <= c["DAG_MAX_COLUMN_TILES"] and nt <= c["DAG_MAX_NT"]:
            return q
    return 0


def test_constants_are_the_ones_the_cases_were_chosen_for(consts):
    assert consts == dict(CHOL_MAXB=16, DAG_MAX_NB=8, DAG_MAX_NT=32, DAG_MAX_COLUMN_TILES=288, ROWSTATS_MAXB=16, SYRK_MAXB=16,
                          LSM_FUSED_MAXL=16, MO_MAXT=16, MC_KMAX=64, MC_TILE=2048)
    capi = open(os.path.join(CSRC, "agp_capi.hip")).read()
    # the dispatch of lsm_local_all: one instantiation per power of two up to LSM_FUSED_MAXL
    assert [int(v) for v in re.findall(r"AGP_LSM_LAUNCH\((\d+)\);", capi)] == [1, 2, 4, 8, 16]


@pytest.mark.parametrize("K", list(MK.ANALYTIC_CASES))
def test_analytic_case_reaches_what_it_claims(consts, K):
    c, claim = consts, MK.ANALYTIC_CASES[K]
    m, B = MK.ANALYTIC["m"], MK.ANALYTIC["B"]
    assert _rup(m) == 128
    lg = None if K > c["LSM_FUSED_MAXL"] else _pow2_at_least(K, 1)
    assert lg == claim["lg"]
    nb = _dag_nb(c, m, B)
    assert nb == 8
    nchunks = -(-K // nb)
    assert _chunks(K, -(-K // nchunks)) == claim["dag"]         # balanced chunks on the task graph
    assert _chunks(K, c["CHOL_MAXB"]) == claim["plain"]         # AGP_CHOL_DAG=0: batches of CHOL_MAXB
    assert _chunks(K, c["ROWSTATS_MAXB"]) == claim["rowstats"]
    assert (1 < K <= c["SYRK_MAXB"]) == claim["eta_batched"]


def test_analytic_cases_cover_every_seam(consts):
    cases = MK.ANALYTIC_CASES
    assert {v["lg"] for v in cases.values()} >= {2, 8, 16, None}
    assert any(v["lg"] is not None and v["lg"] > K for K, v in cases.items())      # idle lanes inside a point's group
    assert any(len(set(v["dag"])) > 1 for v in cases.values())                     # unequal task-graph chunks
    assert consts["LSM_FUSED_MAXL"] + 1 in cases and consts["ROWSTATS_MAXB"] in cases and consts["ROWSTATS_MAXB"] + 1 in cases
    for K in MK.NO_TASK_GRAPH_KS:
        assert K in cases
    assert cases[16]["plain"] == (consts["CHOL_MAXB"],) and cases[17]["plain"] == (consts["CHOL_MAXB"], 1)
    assert MK.VGP10["K"] == MK.HYPER10["K"] == 10 and _rup(MK.VGP10["N"]) == 128
    assert MK.MO16["T"] == consts["MO_MAXT"]


@pytest.mark.parametrize("K", list(MK.MC_POINT_CASES) + list(MK.MC_TRAJECTORY_KS))
def test_mc_case_reaches_what_it_claims(consts, K):
    claim = MK.MC_POINT_CASES.get(K) or MK.MC_TRAJECTORY_KS[K]
    P = _pow2_at_least(K, 2)
    assert 2 <= K <= consts["MC_KMAX"]
    assert dict(P=P, G=64 // P, TS=consts["MC_TILE"] // K) == claim
    if K in MK.MC_POINT_CASES:
        ts = claim["TS"]
        assert MK.mc_nmc(K) == (1, ts, ts + 1, 1000) and 1000 > ts + 1


def test_mc_cases_cover_every_seam(consts):
    Ps = {v["P"] for v in MK.MC_POINT_CASES.values()}
    assert Ps == {4, 8, 16, 32, 64}
    for P in (8, 16, 32, 64):  # at every P from 8 on, one K with idle lanes and one without
        ks = [K for K, v in MK.MC_POINT_CASES.items() if v["P"] == P]
        assert any(K < P for K in ks) and (P == 8 or any(K == P for K in ks)), P
    assert consts["MC_KMAX"] in MK.MC_POINT_CASES
    assert {c["K"] for c in CS.VGP_CASES.values()} >= set(MK.MC_TRAJECTORY_KS)
    assert 10 in {CS.sparse_K(c) for c in CS.SPARSE_CASES.values()}


@pytest.mark.parametrize("K", list(MK.MC_POINT_CASES))
def test_mc_engineered_points_tie_exactly(K):
    import _mcvi_ref as M

    c, mu, var = MK.mc_point_inputs(K)
    assert mu.shape == var.shape == (K, MK.MC_POINTS) and c.shape == (MK.MC_POINTS,) and np.all((c >= 0) & (c < K))
    assert np.all(var[:, 6:9] == 0.0) and np.all(mu[:, 6] == mu[0, 6]) and np.all(mu[:, 7] == mu[0, 7]) and (c[6], c[7]) == (0, K - 1)
    assert mu[K - 2, 8] == mu[K - 1, 8] and (K == 2 or np.max(mu[:K - 2, 8]) < mu[K - 1, 8]) and c[8] == K - 1
    # the restatement breaks the ties at the first maximum: softmax, K equal entries -> g of the first-maximum class 0 is
    # (K - 1) / K formed as (sum of the others) / total, of class K - 1 it is 1 - 1 / K
    eps = M.normals(CS.SEED, 5, M.STREAM_GRAD, 1, K)  # (one draw: the mean rounds nothing)
    ell, g, h, _ = M.expectations("softmax", c, mu, var, eps)
    assert g[0, 6] == (K - 1.0) / K and g[K - 1, 7] == 1.0 - 1.0 / K and ell[6] == ell[7] == -np.log1p(K - 1.0)
    for link in M.LINKS:
        out = M.expectations(link, c, mu, var, eps)
        assert all(np.all(np.isfinite(a)) for a in out[:3])


@pytest.mark.parametrize("K", list(MK.ANALYTIC_CASES))
def test_every_class_in_every_minibatch_and_finite_oracle(K):
    X, y, Z, idx, Xt = MK.analytic_data(K)
    assert sorted(set(y)) == list(range(1, K + 1))
    for ib in idx:
        assert len(ib) == MK.ANALYTIC["B"] and sorted(set(y[ib])) == list(range(1, K + 1))
    o = MK.analytic_oracle(K)
    assert len(o["elbo"]) == MK.ANALYTIC["steps"] and np.all(np.isfinite(o["elbo"]))
    for g in o["model"].latents:
        assert all(np.all(np.isfinite(a)) for a in (g.mu, g.Sigma, g.eta1, g.eta2))
    assert np.all(np.isfinite(o["mean"])) and np.all(o["var"] > 0) and np.allclose(o["proba"].sum(axis=1), 1.0, atol=1e-12)
    assert o["mean"].shape == (K, MK.ANALYTIC["n_test"])


def test_related_cases_have_every_class_and_a_finite_oracle():
    from _vgp_ref import VGPRef
    from oracle import agp_ref as R

    X, y = MK.vgp10_data()
    assert sorted(set(y)) == list(range(1, 11))
    lik = R.LogisticSoftMaxLikelihood(10)
    ref = VGPRef(R.Kernel("sqexponential", MK.VGP10["scale"], MK.VGP10["variance"]), lik, X)
    yt = R.treat_labels(y, lik)
    for _ in range(MK.VGP10["steps"]):
        ref.step(yt)
    assert np.isfinite(ref.elbo(yt)) and all(np.all(np.isfinite(ref.mu[k])) and np.all(np.isfinite(ref.Sigma[k])) for k in range(10))
    X, y, Z, idx = MK.hyper10_data()
    assert all(sorted(set(y[ib])) == list(range(1, 11)) for ib in idx)
    mr = MK.hyper10_oracle()
    var = [g.kernel.sigma2 for g in mr.latents]
    assert np.all(np.isfinite(var)) and len({round(v, 12) for v in var}) == 10  # the per-latent kernels differ after a hyper step
    assert all(np.all(np.isfinite(g.mu)) and np.all(np.isfinite(g.Z)) for g in mr.latents)


def test_mosvgp_case_is_finite_and_cycles_the_likelihoods():
    X, ys, kinds, A, Zs, idx, Xt = MK.mo16_data()
    assert len(ys) == len(kinds) == MK.MO16["T"] == 16 and len(Zs) == MK.MO16["Q"] and A.shape == (16, 5)
    assert kinds[:4] == list(MK.MO_KINDS) and kinds[12:] == list(MK.MO_KINDS)
    assert all(set(np.unique(ys[t])) == {-1.0, 1.0} for t in range(16) if kinds[t] == "logistic")
    o = MK.mo16_oracle()
    assert np.all(np.isfinite(o["elbo"])) and np.all(np.isfinite(o["mean"])) and np.all(o["var"] > 0)
    assert all(np.all(np.isfinite(g.eta2)) for g in o["model"].latents)


@pytest.mark.parametrize("K", MK.LPD_KS)
def test_lpd_inputs(K):
    import _lpd_ref as Rf

    c, mu, var = MK.lpd_inputs(K)
    assert mu.shape == (K, MK.LPD_POINTS) and np.all(np.sum(np.abs(mu) == 800.0, axis=0) == 1) and np.all(np.abs(mu) <= 800.0)
    assert np.all(np.sort(np.abs(mu), axis=0)[:-1] <= 30.0)
    for name in Rf.MULTI:
        ref = Rf.lpd_np((name, K), c, mu, var)
        assert np.all(np.isfinite(ref)) and np.min(ref) < -700.0 and np.max(ref) <= 0.0
