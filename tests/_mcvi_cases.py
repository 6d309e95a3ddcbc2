"""The inputs of the MCIntegrationVI parity tests, shared by the CPU suite (which asserts the margin condition on every one of them,
tests/test_mcvi_host.py) and the GPU suite (tests/test_gpu_mcvi.py).  A restated trajectory is computed once per case and cached."""
import functools

import numpy as np

import _mcvi_ref as M
import _nvi_ref as Q
from oracle import agp_ref as R

NMC, SEED = 200, 2024
KVAR, SCALE, JITTER = 1.5, 2.0, 1e-4  # 1.5 SqExponential o ScaleTransform(2): spread 1 against a length scale of 1 / 2
OPTS = {"descent": ("descent", 0.1), "adam": ("adam", 0.01)}  # natural + Descent(0.1), classical + ADAM(0.01)
VGP_STEPS = 12


def _vgp_cases():
    out = {}
    for link in M.LINKS:
        for natural, opt in ((True, "descent"), (False, "adam")):
            out[f"{link}-40-{'nat' if natural else 'cla'}-{opt}"] = dict(link=link, N=40, K=3, natural=natural, opt=opt)
    out["softmax-70-k2-nat-descent"] = dict(link="softmax", N=70, K=2, natural=True, opt="descent")  # crosses the 64-tile edge
    # class counts at which k_mc_local changes shape (tests/_multiclass_cases.py): K = 10 -> 16 lanes per draw, K = 17 -> 32
    out["softmax-40-k10-nat-descent"] = dict(link="softmax", N=40, K=10, natural=True, opt="descent")
    out["logisticsoftmax-70-k17-cla-adam"] = dict(link="logisticsoftmax", N=70, K=17, natural=False, opt="adam")
    return out


VGP_CASES = _vgp_cases()


def classes(X, K, rng):
    """class indices 0 .. K-1 from K noisy score functions of the inputs (every class occurs)"""
    s = np.stack([np.sin(2 * X[:, 0] + 2.1 * k) + 0.5 * np.cos(1.5 * X[:, 1] - k) for k in range(K)], axis=1)
    c = np.argmax(s + 0.3 * rng.standard_normal(s.shape), axis=1)
    c[:K] = np.arange(K)
    return c


def data(case, D=2, seed=5):
    rng = np.random.default_rng(seed + case["N"])
    X = rng.standard_normal((case["N"], D))
    return X, classes(X, case["K"], rng)


def make_opt(name):
    kind, eta = OPTS[name]
    return lambda: Q.make_rule(kind, eta)


def kernel():
    return R.Kernel("sqexponential", SCALE, KVAR)


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """the restated steps of a VGP case: per step and latent mu and Sigma, the ELBO after every step, the alpha tuples, the
    counters per latent, the smallest margin"""
    case = VGP_CASES[name]
    X, c = data(case)
    ref = M.McRef(kernel(), case["link"], case["K"], X, NMC, SEED, make_opt(case["opt"]), natural=case["natural"], jitter=JITTER)
    mus, Sigmas, elbos = [], [], []
    for _ in range(VGP_STEPS):
        ref.step(c)
        mus.append([r.mu.copy() for r in ref.lat])
        Sigmas.append([r.Sigma.copy() for r in ref.lat])
        elbos.append(ref.elbo(c))
    return dict(ref=ref, mu=mus, Sigma=Sigmas, elbo=elbos, alphas=list(ref.alphas), counters=ref.counters(), margin=min(ref.margins))


# ---- the sparse model: m = 70 inducing points, N = 400, D = 3, K = 3 (one case: K = 10), 10 steps; MCIntegrationVI (B = N) and
# MCIntegrationSVI(150) on the restatement's index stream ------------------------------------------------------------------------------
SPARSE = dict(m=70, N=400, D=3, K=3, B=150, steps=10)
SPARSE_CASES = {f"{link}-{'svi' if stoch else 'vi'}-{'nat' if natural else 'cla'}-{opt}": dict(link=link, stoch=stoch, natural=natural, opt=opt)
                for link, stoch, natural, opt in (("softmax", False, True, "descent"), ("logisticsoftmax", False, False, "adam"),
                                                  ("softmax", True, False, "adam"), ("logisticsoftmax", True, True, "descent"))}
SPARSE_CASES["softmax-svi-k10-nat-descent"] = dict(link="softmax", stoch=True, natural=True, opt="descent", K=10)


def sparse_K(case):
    return case.get("K", SPARSE["K"])


def sparse_data(case):
    rng = np.random.default_rng(23)
    N, D, m = SPARSE["N"], SPARSE["D"], SPARSE["m"]
    X = rng.standard_normal((N, D))
    c = classes(X, sparse_K(case), rng)
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [np.sort(rng.choice(N, SPARSE["B"], replace=False)) for _ in range(SPARSE["steps"])] if case["stoch"] else None
    return X, c, Z, idx


@functools.lru_cache(maxsize=None)
def sparse_trajectory(name):
    case = SPARSE_CASES[name]
    X, c, Z, idx = sparse_data(case)
    ref = M.McSparseRef(kernel(), case["link"], sparse_K(case), Z, NMC, SEED, make_opt(case["opt"]), natural=case["natural"], jitter=JITTER)
    rho = SPARSE["N"] / SPARSE["B"] if case["stoch"] else 1.0
    mus, Sigmas, elbos = [], [], []
    for it in range(SPARSE["steps"]):
        ib = idx[it] if idx is not None else np.arange(len(X))
        ref.step(c[ib], X[ib], rho)
        mus.append([r.mu.copy() for r in ref.lat])
        Sigmas.append([r.Sigma.copy() for r in ref.lat])
        elbos.append(ref.elbo(c[ib], X[ib], rho))
    return dict(ref=ref, mu=mus, Sigma=Sigmas, elbo=elbos, alphas=list(ref.alphas), counters=ref.counters(), margin=min(ref.margins))


# ---- the expectation kernel point by point: 500 points, |mu| up to 30, var from 1e-12 to 1e2, points at var = 0 -------------------
def point_inputs(K, P=500, seed=7):
    rng = np.random.default_rng(seed + K)
    mu = rng.uniform(-30, 30, (K, P))
    var = 10.0 ** rng.uniform(-12, 2, (K, P))
    var[:, :4] = np.array([1e-12, 1e2, 0.0, 0.0])[None, :]
    var[0, 4], var[K - 1, 5] = 0.0, 0.0  # (and single latents at var = 0)
    mu[:, 3] = 30.0 * np.where(np.arange(K) == 0, 1.0, -1.0)  # the extreme corner at var = 0
    c = rng.integers(0, K, P)
    c[3] = 1  # (the unlikely class there: log p = -60)
    return c, mu, var
