"""CPU, oracle only: the inputs of tests/_online_cases.py have the properties tests/test_gpu_online_edges.py relies on, so that a
later edit of a case cannot silently make a device test vacuous.

* every lattice stream reaches exactly its prescribed sequence of m under the real OIPS rule, with the stated accept / reject margins
  (the selection cannot depend on the precision or on who computes the kernel values);
* every scripted case is well conditioned (cond(K) <= 1e3), keeps -2 eta2 positive definite after every batch, and has
  tr K~_a >= 1 at every hand-over after the first (the terms that vanish when Z_a is a subset of Z do not vanish);
* every case discriminates: an oracle that keeps only the first 64 entries of Z_a, invD_a and eta1_a -- what a one-tile loop bound
  in the streaming prior would compute -- differs from the true oracle at every hand-over with ma > 64 by at least 1e-3 in eta2
  (relative, max norm) and in the ELBO (relative)."""
import copy

import numpy as np
import pytest

import _online_cases as OC
from _liks import oracle_lik
from oracle import agp_ref as R


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _oracle(c, Zalg, **kw):
    lik = oracle_lik(R, c["lik"])
    if c["lik"] == "logisticsoftmax":
        lik.class_mapping = [1, 2, 3]
    return R.OnlineSVGP(OC.oracle_kernel(R, c), lik, Zalg, **kw)


class _OneTile(R.OnlineSVGP):
    """the streaming prior cut to its first 64 old inducing points; the local update under the old posterior keeps all of them"""

    def _roll(self, X):
        super()._roll(X)
        for g in self.latents:
            g["Za_all"] = g["Za"]
            g["Za"], g["invDa"], g["prev_eta1"] = g["Za"][:OC.TILE], g["invDa"][:OC.TILE, :OC.TILE], g["prev_eta1"][:OC.TILE]

    def _old_matrices(self, X):
        out = []
        for g in self.latents:
            K, L = R.compute_K(g["kernel"], g["Za_all"], self.jitter)
            out.append(R.compute_kappa(g["kernel"], X, g["Za_all"], L, self.jitter))
        return out


def _discriminates(mr, c, b, Zalg_next):
    """train batch b on a copy of `mr` (the true state before the batch) cut to one tile; return the copy for comparison"""
    cut = copy.deepcopy(mr)
    cut.__class__ = _OneTile
    cut.Zalg = Zalg_next
    cut.train(c["Xs"][b], c["ys"][b], c["iters"])
    return cut


@pytest.mark.parametrize("D", [1, 2, 3])
def test_lattice_stream_selection_and_margins(D):
    c = OC.growth_case(D)
    ker, alg = OC.oracle_kernel(R, c), R.OIPS(OC.RHO)
    Z, worst_acc, best_rej = None, 0.0, np.inf
    for b, X in enumerate(c["Xs"]):
        assert len(X) == OC.GROWTH_BS[b]
        Zs = [X[0]] if Z is None else list(Z)  # the sequential scan of the rule, with the margins recorded
        for x in (X[1:] if Z is None else X):
            kmax = float(np.max(ker.matrix(x[None, :], np.stack(Zs))))
            if kmax < OC.RHO:
                Zs.append(x)
                worst_acc = max(worst_acc, kmax)
            else:
                best_rej = min(best_rej, kmax)
        Z = alg.init(X, ker) if Z is None else alg.update(Z, X, ker)
        assert np.array_equal(Z, np.stack(Zs))
        assert len(Z) == c["m_seq"][b], (b, len(Z))
        assert np.array_equal(Z, OC.growth_sets(D)[b])
    print(f"D = {D}: largest accepted kernel value {worst_acc:.4f}, smallest rejected {best_rej:.4f}")
    assert worst_acc <= 0.4 and best_rej >= 1.1
    assert [(a, m) for a, m, *_ in OC.combos(c)] == [(40, 63), (63, 64), (64, 65), (65, 65), (65, 128), (128, 130)]


@pytest.mark.parametrize("D,likname", [(1, "logistic"), (2, "logistic"), (3, "logistic"), (2, "gaussian"), (2, "logisticsoftmax")])
def test_growth_case_discriminates(D, likname):
    c = OC.growth_case(D, likname)
    mr = _oracle(c, R.OIPS(OC.RHO))
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        ma = len(mr.latents[0]["Z"]) if b else 0
        cut = _discriminates(mr, c, b, R.OIPS(OC.RHO)) if ma > OC.TILE else None
        mr.train(X, y, c["iters"])
        assert np.linalg.cond(mr.latents[0]["K"]) <= 1e3
        if cut is not None:
            yt = R.treat_labels(y, mr.likelihood)
            d2 = max(_rel(gc["eta2"], g["eta2"]) for gc, g in zip(cut.latents, mr.latents))
            de = abs(cut.elbo(yt) - mr.elbo(yt)) / abs(mr.elbo(yt))
            print(f"{c['name']} batch {b} ma = {ma}: one-tile prior differs by {d2:.2e} in eta2, {de:.2e} in the ELBO")
            assert d2 >= 1e-3 and de >= 1e-3, (b, d2, de)


SCRIPTED = [("A", "logistic", 2, "matern52", {}), ("A", "logisticsoftmax", 2, "matern52", {}),
            ("B", "logistic", 2, "matern52", {}), ("B", "logisticsoftmax", 2, "matern52", {}),
            ("A", "gaussian", 9, "sqexponential", {}),
            ("A", "logistic", 2, "matern52", dict(k_opt=0.01, z_opt=0.001)), ("A", "logistic", 2, "matern52", dict(B=60)),
            ("B", "logistic", 2, "matern52", dict(jitter=1e-3)), ("B", "logisticsoftmax", 2, "matern52", dict(jitter=1e-3))]


@pytest.mark.parametrize("seq,likname,D,kind,kw", SCRIPTED, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_scripted_case_is_sound_and_discriminates(seq, likname, D, kind, kw):
    c = OC.scripted_case(seq, likname, D, kind, B=kw.get("B", OC.B_SCRIPTED))
    kw = {k: (R.Adam(v) if k.endswith("_opt") else v) for k, v in kw.items() if k != "B"}
    nl = oracle_lik(R, likname).n_latent
    mr = _oracle(c, OC.Scripted([c["sets"]] * nl), **kw)
    for b, (X, y) in enumerate(zip(c["Xs"], c["ys"])):
        ma = len(mr.latents[0]["Z"]) if b else 0
        cut = None
        if ma > OC.TILE:
            alg = OC.Scripted([c["sets"]] * nl)
            alg.calls = b * nl
            cut = _discriminates(mr, c, b, alg)
        mr.train(X, y, c["iters"])
        assert len(mr.latents[0]["Z"]) == c["m_seq"][b]
        for g in mr.latents:
            assert np.linalg.cond(g["K"]) <= 1e3, (b, np.linalg.cond(g["K"]))
            assert np.min(np.linalg.eigvalsh(-2.0 * g["eta2"])) > 0.0
            if b:
                assert np.trace(g["Kt_a"]) >= 1.0, (b, np.trace(g["Kt_a"]))
                assert not set(map(tuple, g["Za"])) <= set(map(tuple, g["Z"]))  # the old set is not inside the new one
        if cut is not None:
            yt = R.treat_labels(y, mr.likelihood)
            d2 = max(_rel(gc["eta2"], g["eta2"]) for gc, g in zip(cut.latents, mr.latents))
            de = abs(cut.elbo(yt) - mr.elbo(yt)) / abs(mr.elbo(yt))
            print(f"{c['name']} batch {b} ma = {ma}: one-tile prior differs by {d2:.2e} in eta2, {de:.2e} in the ELBO; "
                  f"cond(K) {np.linalg.cond(mr.latents[0]['K']):.1f}, tr K~_a {np.trace(mr.latents[0]['Kt_a']):.1f}")
            assert d2 >= 1e-3 and de >= 1e-3, (b, d2, de)
    assert [(a, m) for a, m, *_ in OC.combos(c)] == list(zip(c["m_seq"][:-1], c["m_seq"][1:]))
