"""The inputs of the QuadratureVI parity tests, shared by the CPU suite (which asserts the margin condition on every one of them,
tests/test_nvi_host.py) and the GPU suite (tests/test_gpu_nvi.py).  A restated trajectory is computed once per case and cached."""
import functools

import numpy as np

import _nvi_ref as Q
from _liks import labels, oracle_lik
from oracle import agp_ref as R

STEPS = 20
LIKS = ("logistic", "studentt", "laplace")
OPTS = {"descent": ("descent", 0.1), "momentum": ("momentum", 1e-5), "adam": ("adam", 0.01)}  # Descent(0.1), the default, ADAM(0.01)


# The grid of the parity cases is likelihood x N x {natural, classical} x optimiser, all 36 cells.  Seven cells run a SHORTER horizon
# than STEPS, because beyond it the restated chain itself is no reference (tests/test_nvi_host.py asserts each statement on the
# restatement, and that the chain is well posed -- margin condition, a 1e-14 perturbation stays below 1e-10 -- up to the short horizon):
#   classical x Descent(0.1), 8 steps   the classical gradient of eta2 has the size of K^-1, far beyond what a step of 0.1 tolerates.
#                                       At N = 130 the ELBO reaches -1e59 by step 20; at N = 63 the chain stays bounded but a
#                                       perturbation of 1e-14 after its first step grows beyond 1e-9 by step 20
#   logistic-130 natural x ADAM, 10 steps   ADAM moves every entry of the 130 x 130 Sigma by about eta = 0.01 per step, a perturbation of
#                                       norm ~1.3 > lambda_min: from step 12 on the chain runs along the boundary of the cone
#                                       (margin 5e-8, later 5e-10, < 1e-7)
SHORT = {}  # name -> (steps, what happens by step STEPS)


def _vgp_cases():
    out = {}
    for N in (63, 130):  # a 64-tile filled short, and crossed
        for lik in LIKS:
            for natural in (True, False):
                for opt in OPTS:
                    name = f"{lik}-{N}-{'nat' if natural else 'cla'}-{opt}"
                    out[name] = dict(lik=lik, N=N, natural=natural, opt=opt, mean=None, kind="sqexponential", scale=3.0)
                    if not natural and opt == "descent":
                        SHORT[name] = (8, "diverges" if N == 130 else "unstable")
                    elif name == "logistic-130-nat-adam":
                        SHORT[name] = (10, "margin")
    out["logistic-130-nat-descent-constmean"] = dict(lik="logistic", N=130, natural=True, opt="descent", mean=0.3,
                                                     kind="sqexponential", scale=3.0)
    out["studentt-63-nat-descent-empmean"] = dict(lik="studentt", N=63, natural=True, opt="descent", mean="empirical",
                                                  kind="sqexponential", scale=3.0)
    out["laplace-130-nat-descent-ardmatern52"] = dict(lik="laplace", N=130, natural=True, opt="descent", mean=None, kind="matern52",
                                                      scale=(1.5, 2.5, 0.8))
    return out


def steps_of(name):
    return SHORT[name][0] if name in SHORT else STEPS


VGP_CASES = _vgp_cases()
FIXED_POINT = dict(N=40, D=2, steps=300)  # Logistic, natural, Descent(0.1), n = 100, kernel 2 SqExponential, jitter 1e-4


def data(case, D=3, seed=3):
    rng = np.random.default_rng(seed + case["N"])
    X = rng.standard_normal((case["N"], D))  # (spread 1 against a length scale of 1 / 3: K + jitt I is well conditioned)
    f = np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] ** 2 - 0.7
    y = labels(case["lik"], f, X, rng)
    mean = case["mean"]
    if isinstance(mean, str):  # EmpiricalMean: one value per training point
        mean = 0.2 * np.cos(4 * X[:, 2])
    return X, y, mean


def make_ref(case, n=100):
    X, y, mean = data(case)
    lik = oracle_lik(R, case["lik"])
    kind, eta = OPTS[case["opt"]]
    scale = case["scale"] if np.isscalar(case["scale"]) else np.asarray(case["scale"], dtype=np.float64)
    mu0 = None if mean is None else np.full(len(X), mean) if np.isscalar(mean) else np.asarray(mean, dtype=np.float64)
    ref = Q.NviRef(R.Kernel(case["kind"], scale, 1.5), lik, X, n=n, opt=Q.make_rule(kind, eta), natural=case["natural"], mu0=mu0)
    return X, y, mean, R.treat_labels(y, lik).astype(np.float64), ref


@functools.lru_cache(maxsize=None)
def trajectory(name, steps=None):
    """the restated steps of a case (its own horizon unless given): mu, Sigma and the ELBO after every step, the alpha history, the
    counters, the margins"""
    X, y, mean, yt, ref = make_ref(VGP_CASES[name])
    mus, Sigmas, elbos = [], [], []
    for _ in range(steps_of(name) if steps is None else steps):
        ref.step(yt)
        mus.append(ref.mu.copy())
        Sigmas.append(ref.Sigma.copy())
        elbos.append(ref.elbo(yt))
    return dict(ref=ref, mu=mus, Sigma=Sigmas, elbo=elbos, alphas=list(ref.alphas), halvings=ref.halvings, rejected=ref.rejected,
                margin=min(ref.margins), node_margin=min(ref.node_margins) if ref.node_margins else None)


def sensitivity(name, steps, eps=1e-14):
    """largest relative difference in (mu, Sigma) after `steps` steps between the restated chain and the same chain with mu and
    Sigma perturbed by eps (relative, alternating signs) after its first step"""
    case = VGP_CASES[name]
    chains = []
    for perturb in (False, True):
        X, y, mean, yt, ref = make_ref(case)
        for it in range(steps):
            ref.step(yt)
            if perturb and it == 0:
                sg = np.where(np.arange(len(ref.mu)) % 2, 1.0, -1.0)
                ref.mu = ref.mu + eps * (1.0 + np.abs(ref.mu)) * sg
                ref.Sigma = ref.Sigma + eps * np.abs(ref.Sigma) * np.outer(sg, sg)
        chains.append(ref)
    a, b = chains
    return max(float(np.max(np.abs(a.mu - b.mu)) / np.max(np.abs(a.mu))), float(np.max(np.abs(a.Sigma - b.Sigma)) / np.max(np.abs(a.Sigma))))


def fixed_point_problem():
    rng = np.random.default_rng(11)
    N, D = FIXED_POINT["N"], FIXED_POINT["D"]
    X = rng.standard_normal((N, D))
    y = np.sign(np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(N))
    y[y == 0] = 1.0
    return X, y


@functools.lru_cache(maxsize=None)
def fixed_point_reference():
    X, y = fixed_point_problem()
    ref = Q.NviRef(R.Kernel("sqexponential", 1.0, 2.0), R.LogisticLikelihood(), X, n=100, opt=R.Descent(0.1), natural=True)
    for _ in range(FIXED_POINT["steps"]):
        ref.step(y)
    return ref, y


# ---- the sparse model: m = 70 inducing points, N = 400, D = 3, 15 steps; QuadratureVI (B = N) and QuadratureSVI(150) on one index
# stream per case (natural gradient with Descent(0.1), classical gradient with ADAM(0.01)) -------------------------------------------
SPARSE = dict(m=70, N=400, D=3, B=150, steps=15)
SPARSE_CASES = {f"{lik}-{'svi' if stoch else 'vi'}-{'nat' if natural else 'cla'}-{opt}": dict(lik=lik, stoch=stoch, natural=natural, opt=opt)
                for lik in LIKS for stoch in (False, True) for natural, opt in ((True, "descent"), (False, "adam"))}


def sparse_data(case):
    rng = np.random.default_rng(17)
    N, D, m = SPARSE["N"], SPARSE["D"], SPARSE["m"]
    X = rng.standard_normal((N, D))
    f = np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] ** 2 - 0.7
    y = labels(case["lik"], f, X, rng)
    Z = X[rng.permutation(N)[:m]].copy()
    idx = [np.sort(rng.choice(N, SPARSE["B"], replace=False)) for _ in range(SPARSE["steps"])] if case["stoch"] else None
    return X, y, Z, idx


@functools.lru_cache(maxsize=None)
def sparse_trajectory(name):
    case = SPARSE_CASES[name]
    X, y, Z, idx = sparse_data(case)
    lik = oracle_lik(R, case["lik"])
    yt = R.treat_labels(y, lik).astype(np.float64)
    kind, eta = OPTS[case["opt"]]
    ref = Q.NviSparseRef(R.Kernel("sqexponential", 3.0, 1.5), lik, Z, n=100, opt=Q.make_rule(kind, eta), natural=case["natural"])
    rho = SPARSE["N"] / SPARSE["B"] if case["stoch"] else 1.0
    mus, Sigmas, elbos = [], [], []
    for it in range(SPARSE["steps"]):
        ib = idx[it] if idx is not None else np.arange(len(X))
        ref.step(X[ib], yt[ib], rho)
        mus.append(ref.mu.copy())
        Sigmas.append(ref.Sigma.copy())
        elbos.append(ref.elbo(X[ib], yt[ib], rho))
    return dict(ref=ref, mu=mus, Sigma=Sigmas, elbo=elbos, alphas=list(ref.alphas), halvings=ref.halvings, rejected=ref.rejected,
                margin=min(ref.margins), node_margin=min(ref.node_margins) if ref.node_margins else None)
