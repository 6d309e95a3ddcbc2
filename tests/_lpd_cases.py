"""Inputs of the streamed log predictive density tests (tests/test_gpu_lpd.py): m = 70 inducing points (the padded size 128 carries
padding), D = 3, 15 AnalyticSVI(150) steps on N = 400 training points on one index stream, then up to 8229 test points drawn from
the same generator.  The trained oracle of a case and its moments at the test points are computed once and cached; nothing mutates
them."""
import functools

import numpy as np

import _lpd_ref as Rf
from _liks import agp_lik, labels, oracle_lik
from oracle import agp_ref as R

M, D, B, STEPS, NTRAIN, NMAX = 70, 3, 150, 15, 400, 8229
NS = (1, 15, 16, 17, 4096, 4097, 8229)
KSCALE, KVAR = 3.0, 1.5

# name -> (likelihood, D, kernel kind, scale (scalar or per dimension), prior mean, number of test points)
CASES = {lik: (lik, D, "sqexponential", KSCALE, None, NMAX)
         for lik in ("gaussian", "laplace", "logistic", "bayesiansvm", "studentt", "poisson", "negbinomial", "logisticsoftmax")}
CASES.update({
    "ard-matern52": ("logistic", D, "matern52", (1.5, 2.5, 0.8), None, NMAX),
    "prior-mean": ("logistic", D, "sqexponential", KSCALE, 0.3, NMAX),
    "d130": ("logistic", 130, "sqexponential", 0.25, None, 300),  # beyond the MFMA kernel-matrix kernel's D
})


def _f(X):
    return np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] ** 2 - 0.7


@functools.lru_cache(maxsize=None)
def data(likname, Dd=D, nt=NMAX):
    """(X, y, Z, idx stream) to train on and (Xt, yt) to score"""
    rng = np.random.default_rng(23 + Dd)
    X = rng.standard_normal((NTRAIN, Dd))
    y = labels(likname, _f(X), X, rng)
    Z = X[rng.permutation(NTRAIN)[:M]].copy()
    idx = [np.sort(rng.choice(NTRAIN, B, replace=False)) for _ in range(STEPS)]
    Xt = rng.standard_normal((nt, Dd))
    ft = _f(Xt)
    if likname in ("logistic", "bayesiansvm"):  # (the generator thresholds at the mean of f: the training one)
        yt = (ft + 0.3 * rng.standard_normal(nt) > _f(X).mean()).astype(np.int64)
    elif likname == "logisticsoftmax":
        yt = 1 + np.digitize(ft, np.quantile(_f(X), [0.33, 0.66]))
    else:
        yt = labels(likname, ft, Xt, rng)
    return X, y, Z, idx, Xt, yt


def ref_lik(lik):
    """the oracle's likelihood object (with its CURRENT state) -> the tuple tests/_lpd_ref.py takes"""
    return {"gaussian": lambda: ("gaussian", lik.sigma2), "laplace": lambda: ("laplace", lik.beta), "logistic": lambda: ("logistic",),
            "bayesiansvm": lambda: ("bayesiansvm",), "studentt": lambda: ("studentt", lik.nu, lik.sigma),
            "poisson": lambda: ("poisson", lik.lam), "negbinomial": lambda: ("negbinomial", lik.r),
            "logisticsoftmax": lambda: ("logisticsoftmax", lik.n_class)}[lik.name]()


def treated(lik, y):
    """labels as the device takes them: +-1, counts, reals as float64; 0-based class indices as int32"""
    yt = R.treat_labels(y, lik)
    return np.argmax(yt, axis=1).astype(np.int32) if lik.name == "logisticsoftmax" else np.asarray(yt, dtype=np.float64)


def restated(lt, yt, mu, var, n_nodes=100):
    """lpd[n] of the float64 restatement from moments (mu, var: [n], or [K, n] for a multi-class likelihood)"""
    x, w = Rf.gh_rule(n_nodes)
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if lt[0] not in Rf.MULTI:
        mu, var = mu.reshape(-1), var.reshape(-1)
    return Rf.lpd_np(lt, yt, mu, var, x, w)


@functools.lru_cache(maxsize=None)
def trained_oracle(name, jitter=None):
    """dict: the trained oracle SVGP of a case, the test points, their treated labels, and the restatement fed with the oracle's
    predict_f(cov=True) at all of them"""
    likname, Dd, kind, scale, mean, nt = CASES[name]
    X, y, Z, idx, Xt, yt = data(likname, Dd, nt)
    lik = oracle_lik(R, likname)
    sc = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64)
    kw = {} if jitter is None else {"jitter": jitter}
    ref = R.SVGP(R.Kernel(kind, sc, KVAR), lik, Z, stochastic=True, batchsize=B, **kw)
    if mean is not None:
        for gp in ref.latents:
            gp.mu0 = np.full(M, float(mean))
    ref.train(X, y, STEPS, idx_stream=idx)
    R.treat_labels(y, lik)  # (the class mapping of the training labels)
    ytt = treated(lik, yt)
    mu, var = ref.predict_f(Xt, cov=True)
    lpd = restated(ref_lik(lik), ytt, np.asarray(mu), np.asarray(var))
    return dict(ref=ref, lik=ref_lik(lik), Xt=Xt, y_raw=yt, yt=ytt, lpd=lpd)


def make_model(AGP, name, T=np.float64, **kw):
    """the host mirror's model of a case, trained on the case's index stream"""
    likname, Dd, kind, scale, mean, nt = CASES[name]
    X, y, Z, idx, Xt, yt = data(likname, Dd, nt)
    base = {"sqexponential": AGP.SqExponentialKernel, "matern52": AGP.Matern52Kernel}[kind]()
    tr = AGP.ScaleTransform(float(scale)) if np.isscalar(scale) else AGP.ARDTransform(np.asarray(scale, dtype=np.float64))
    model = AGP.SVGP(KVAR * (base @ tr), agp_lik(AGP, likname), AGP.AnalyticSVI(B), Z, optimiser=False, mean=mean, T=T, **kw)
    AGP.train_(model, X, y, STEPS, idx_stream=idx)
    return model
