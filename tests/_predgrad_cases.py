"""The parity cases of predict_f_grad, shared by the CPU suite (tests/test_predgrad_host.py asserts the conditioning of every one of
them) and the GPU suite (tests/test_gpu_predgrad.py).  A case names a model pair -- the host mirror's model and the oracle model it
is compared with elsewhere -- trained for a few steps on the same data, and a set of test points.  `reference(name)` trains the
oracle side once (cached, never mutated) and returns the per-latent (Z, s, v, kind, a, A) of tests/_predgrad_ref.py, the mixing
matrix of a multi-output model and the test points; `make_model(AGP, name)` builds and trains the device side.

One case per axis value, not the product:  m in {1, 63, 64, 65, 130};  D in {1, 3, 64};  n_t in {1, 255, 4096 + 37};  the three
kernels with ScaleTransform and ARDTransform;  SVGP Gaussian / Logistic with a constant prior mean, LogisticSoftMax K = 3, VGP and GP
at N = 65, MOSVGP with 2 tasks and 3 latents, a QuadratureVI SVGP, an OnlineSVGP after two batches.

Inputs: points ~ spread * N(0, I), scales chosen so that a typical scaled squared distance to the nearer inducing points is of order
one and K + jitt I stays well conditioned (spread 1 against a length scale 1 / 3 at D = 3; the points spread out at D = 1; a long
length scale at D = 64, where all distances are alike).  tests/test_predgrad_host.py holds every case to that.
"""
import functools

import numpy as np

import _predgrad_ref as G
from _liks import agp_lik, labels, oracle_lik
from oracle import agp_ref as R

NTRAIN, B, STEPS = 300, 100, 5
KVAR = 1.5
KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel", "matern32": "Matern32Kernel",
           "exponential": "ExponentialKernel"}
ARD64 = tuple(0.18 * (1.0 + 0.3 * np.cos(np.arange(64))))

# name -> model family, likelihood, m (N for the full models), D, n_t, kernel kind, scale (scalar: ScaleTransform, tuple: ARDTransform),
# spread of the inputs, constant prior mean
CASES = {
    "svgp-gaussian-m130-nt4133-sq-scale": dict(model="svgp", lik="gaussian", m=130, D=3, nt=4096 + 37, kind="sqexponential", scale=3.0,
                                                spread=1.0, mean=0.3),
    "svgp-logistic-m65-m32-ard": dict(model="svgp", lik="logistic", m=65, D=3, nt=255, kind="matern32", scale=(1.5, 2.5, 0.8),
                                      spread=1.0, mean=0.3),
    "svgp-gaussian-m1-nt1-m52-scale": dict(model="svgp", lik="gaussian", m=1, D=3, nt=1, kind="matern52", scale=0.6, spread=1.0,
                                           mean=None),
    "svgp-logistic-d1-m63-m52-ard": dict(model="svgp", lik="logistic", m=63, D=1, nt=255, kind="matern52", scale=(2.0,), spread=8.0,
                                         mean=None),
    "svgp-gaussian-d64-m64-sq-ard": dict(model="svgp", lik="gaussian", m=64, D=64, nt=255, kind="sqexponential", scale=ARD64,
                                         spread=1.0, mean=None),
    "svgp-softmax3-m65-sq-scale": dict(model="svgp", lik="logisticsoftmax", m=65, D=3, nt=255, kind="sqexponential", scale=3.0,
                                       spread=1.0, mean=None),
    "vgp-n65-m32-scale": dict(model="vgp", lik="logistic", m=65, D=3, nt=255, kind="matern32", scale=3.0, spread=1.0, mean=None),
    "gp-n65-sq-ard": dict(model="gp", lik="gaussian", m=65, D=3, nt=255, kind="sqexponential", scale=(3.0, 2.0, 4.0), spread=1.0,
                          mean=None),
    "mosvgp-2tasks-3latents-m63": dict(model="mosvgp", lik=None, m=63, D=3, nt=255, kind="sqexponential", scale=3.0, spread=1.0,
                                       mean=None),
    "svgp-quadrature-m65": dict(model="quad", lik="logistic", m=65, D=3, nt=255, kind="sqexponential", scale=3.0, spread=1.0,
                                mean=None),
    "online-two-batches": dict(model="online", lik="gaussian", m=None, D=2, nt=255, kind="sqexponential", scale=1.5, spread=None,
                               mean=None),
}
FP32_CASE = "svgp-logistic-m65-m32-ard"


def _f(X):
    return np.sin(2 * X[:, 0] / (1.0 + 0.1 * np.abs(X[:, 0]))) + 0.5 * np.tanh(X[:, -1]) ** 2 - 0.3


def _scale(c):
    return c["scale"] if np.isscalar(c["scale"]) else np.asarray(c["scale"], dtype=np.float64)


def _rkernel(c):
    return R.Kernel(c["kind"], _scale(c), KVAR)


def _akernel(AGP, c):
    tr = AGP.ScaleTransform(float(c["scale"])) if np.isscalar(c["scale"]) else AGP.ARDTransform(_scale(c))
    return KVAR * (getattr(AGP, KERNELS[c["kind"]])() @ tr)


@functools.lru_cache(maxsize=None)
def data(name):
    """dict of the case's training data and test points"""
    c = CASES[name]
    rng = np.random.default_rng(101 + sum(map(ord, name)))
    D, nt = c["D"], c["nt"]
    if c["model"] == "online":  # (the stream of tests/test_gpu_online.py)
        N = 120
        X = rng.random((N, D)) * np.array([5.0, 2.0])
        f = np.sin(2 * X[:, 0]) + 0.5 * np.cos(3 * X[:, -1])
        return dict(X=X, y=labels(c["lik"], f, X, rng), Xt=rng.random((nt, D)) * np.array([5.0, 2.0]))
    N = c["m"] if c["model"] in ("vgp", "gp") else (240 if c["model"] == "mosvgp" else NTRAIN)
    X = c["spread"] * rng.standard_normal((N, D))
    out = dict(X=X, Xt=c["spread"] * rng.standard_normal((nt, D)))
    if c["model"] == "mosvgp":
        out["ys"] = [np.sign(_f(X) + 0.1 * rng.standard_normal(N)), np.cos(X[:, 0]) + 0.1 * rng.standard_normal(N)]
        A = rng.standard_normal((2, 3))
        out["A"] = A / np.linalg.norm(A, axis=1, keepdims=True)
        out["Zs"] = [X[rng.permutation(N)[:c["m"]]].copy() for _ in range(3)]
        out["idx"] = [rng.choice(N, 80, replace=False) for _ in range(STEPS)]
        return out
    out["y"] = labels(c["lik"], _f(X), X, rng)
    if c["model"] in ("svgp", "quad"):
        out["Z"] = X[rng.permutation(N)[:c["m"]]].copy()
        out["idx"] = [np.sort(rng.choice(N, B, replace=False)) for _ in range(STEPS)]
    return out


def _latent(gp, jitter):
    L = gp.L if gp.L is not None else R.compute_K(gp.kernel, gp.Z, jitter)[1]
    return G.latent_parts(gp.kernel, gp.Z, L, gp.mu, gp.Sigma)


@functools.lru_cache(maxsize=None)
def reference(name, jitter=None):
    """dict(parts=[(Z, s, v, kind, a, A) per latent], A=mixing matrix or None, Xt=test points, jitter); jitter: of the SVGP cases
    (None: the reference's Float64 constant; 1e-3 is its Float32 one)"""
    c, d = CASES[name], data(name)
    mixA = None
    if c["model"] == "svgp":
        kw = {} if jitter is None else {"jitter": jitter}
        ref = R.SVGP(_rkernel(c), oracle_lik(R, c["lik"]), d["Z"], stochastic=True, batchsize=B, **kw)
        if c["mean"] is not None:
            for gp in ref.latents:
                gp.mu0 = np.full(c["m"], float(c["mean"]))
        ref.train(d["X"], d["y"], STEPS, idx_stream=d["idx"])
        parts = [_latent(gp, ref.jitter) for gp in ref.latents]
    elif c["model"] == "mosvgp":
        ref = R.MOSVGP(_rkernel(c), [R.LogisticLikelihood(), R.GaussianLikelihood(0.1)], d["Zs"], d["A"].copy(), stochastic=True,
                       batchsize=80)
        ref.train(d["X"], d["ys"], STEPS, idx_stream=d["idx"])
        parts = [_latent(gp, ref.jitter) for gp in ref.latents]
        mixA = ref.A.copy()
    elif c["model"] == "vgp":
        from _vgp_ref import VGPRef

        lik = oracle_lik(R, c["lik"])
        ref = VGPRef(_rkernel(c), lik, d["X"])
        ref.train(R.treat_labels(d["y"], lik), 3)
        parts = [G.latent_parts(ref.kernels[0], ref.X, ref.Ls[0], ref.mu[0], ref.Sigma[0])]
    elif c["model"] == "gp":
        from _gp_ref import GPRef

        ref = GPRef(_rkernel(c), d["X"], d["y"], noise=0.05, opt_noise=False)
        parts = [(ref.X, ref.kernel.scale, ref.kernel.sigma2, ref.kernel.kind, ref.alpha, (ref.Sinv + ref.Sinv.T) / 2)]
    elif c["model"] == "quad":
        import _nvi_ref as Q

        lik = oracle_lik(R, c["lik"])
        ref = Q.NviSparseRef(_rkernel(c), lik, d["Z"], n=100, opt=Q.make_rule("descent", 0.1), natural=True)
        yt = R.treat_labels(d["y"], lik).astype(np.float64)
        for _ in range(4):
            ref.step(d["X"], yt, 1.0)
        parts = [G.latent_parts(ref.kernel, ref.Z, ref.L, ref.mu, ref.Sigma)]
    elif c["model"] == "online":
        ref = R.OnlineSVGP(R.Kernel(c["kind"], c["scale"], 1.2), oracle_lik(R, c["lik"]), R.OIPS(0.7))
        for b in (0, 60):
            ref.train(d["X"][b:b + 60], d["y"][b:b + 60], 3)
        parts = [G.latent_parts(g["kernel"], g["Z"], g["L"], g["mu"], g["Sigma"]) for g in ref.latents]
    else:
        raise ValueError(c["model"])
    return dict(parts=parts, A=mixA, Xt=d["Xt"], jitter=getattr(ref, "jitter", 1e-4))


def restated(name, dtype=np.float64, Xt=None, cov=True, jitter=None):
    """(dmu, dvar): lists over the outputs (latents, or tasks of a multi-output case) of (n_t, D) arrays"""
    ref = reference(name, jitter)
    Xt = ref["Xt"] if Xt is None else Xt
    gs = [G.grads(Xt, *p[:5], p[5] if cov else None, dtype=dtype) for p in ref["parts"]]
    gm, gv = [g[0] for g in gs], [g[1] for g in gs]
    if ref["A"] is not None:
        gm = G.mix(ref["A"], gm)
        gv = G.mix(ref["A"], gv, square=True) if cov else gv
    return gm, gv


def make_model(AGP, name, T=np.float64):
    """the host mirror's model of a case, trained like the oracle side"""
    c, d = CASES[name], data(name)
    if c["model"] == "svgp":
        model = AGP.SVGP(_akernel(AGP, c), agp_lik(AGP, c["lik"]), AGP.AnalyticSVI(B), d["Z"], optimiser=False, mean=c["mean"], T=T)
        AGP.train_(model, d["X"], d["y"], STEPS, idx_stream=d["idx"])
    elif c["model"] == "mosvgp":
        model = AGP.MOSVGP(_akernel(AGP, c), [AGP.LogisticLikelihood(), AGP.GaussianLikelihood(0.1)], AGP.AnalyticSVI(80), d["Zs"],
                           A=d["A"].copy(), Aoptimiser=False, optimiser=False)
        AGP.train_(model, d["X"], d["ys"], STEPS, idx_stream=d["idx"])
    elif c["model"] == "vgp":
        model = AGP.VGP(d["X"], d["y"], _akernel(AGP, c), agp_lik(AGP, c["lik"]), AGP.AnalyticVI(), optimiser=False)
        AGP.train_(model, 3)
    elif c["model"] == "gp":
        model = AGP.GP(d["X"], d["y"], _akernel(AGP, c), noise=0.05, opt_noise=False, optimiser=False)
    elif c["model"] == "quad":
        inf = AGP.QuadratureVI(nGaussHermite=100, optimiser=AGP.Descent(0.1), natural=True)
        model = AGP.SVGP(_akernel(AGP, c), agp_lik(AGP, c["lik"]), inf, d["Z"], optimiser=False)
        AGP.train_(model, d["X"], d["y"], 4)
    elif c["model"] == "online":
        k = 1.2 * (AGP.SqExponentialKernel() @ AGP.ScaleTransform(float(c["scale"])))
        model = AGP.OnlineSVGP(k, agp_lik(AGP, c["lik"]), AGP.AnalyticVI(), AGP.OIPS(0.7), optimiser=False)
        for b in (0, 60):
            AGP.train_online(model, d["X"][b:b + 60], d["y"][b:b + 60], iterations=3)
    else:
        raise ValueError(c["model"])
    return model
