"""Inputs and the oracle restatement of the streamed full-data ELBO (agp_svgp_elbo_stream), shared by the CPU suite
(tests/test_elbo_stream_host.py: the restatement equals SVGP.elbo_fresh) and the GPU suite (tests/test_gpu_elbo_stream.py).

Every case: m = 70 inducing points (so the padded size 128 carries padding), D = 3, 15 AnalyticSVI(150) steps on one index stream
so that the posterior is not the prior.  The trained oracle model of a case is computed once and cached; nothing mutates it."""
import functools
import math

import numpy as np

from _liks import agp_lik, labels, oracle_lik
from oracle import agp_ref as R

M, D, B, STEPS, NMAX, CHUNK = 70, 3, 150, 15, 8229, 4096
KSCALE, KVAR = 3.0, 1.5


def data(likname, N=NMAX, D=D, seed=5):
    """targets in the style of tests/_nvi_cases.py"""
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    f = np.sin(2 * X[:, 0]) + 0.5 * X[:, 1] ** 2 - 0.7
    y = labels(likname, f, X, rng)
    Z = X[rng.permutation(N)[:M]].copy()
    idx = [np.sort(rng.choice(N, min(B, N), replace=False)) for _ in range(STEPS)]
    return X, y, Z, idx


# name -> (likelihood, N the model is trained on, D, kernel kind, scale (scalar or per dimension), elbo_mode, prior mean)
CASES = {
    "logistic": ("logistic", NMAX, D, "sqexponential", KSCALE, "corrected", None),
    "logistic-ref": ("logistic", NMAX, D, "sqexponential", KSCALE, "reference", None),
    "gaussian": ("gaussian", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "studentt": ("studentt", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "laplace": ("laplace", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "laplace-ref": ("laplace", 4133, D, "sqexponential", KSCALE, "reference", None),
    "bayesiansvm": ("bayesiansvm", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "negbinomial": ("negbinomial", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "logisticsoftmax": ("logisticsoftmax", 4133, D, "sqexponential", KSCALE, "corrected", None),
    "logisticsoftmax-ref": ("logisticsoftmax", 4133, D, "sqexponential", KSCALE, "reference", None),
    "ard-matern52": ("logistic", 4133, D, "matern52", (1.5, 2.5, 0.8), "corrected", None),
    "prior-mean": ("logistic", 4133, D, "sqexponential", KSCALE, "corrected", 0.3),
    "d130": ("logistic", 200, 130, "sqexponential", 0.25, "corrected", None),  # beyond the MFMA kernel-matrix kernel's D
}


@functools.lru_cache(maxsize=None)
def trained_oracle(name):
    """(X, y, treated y, Z, idx stream, trained oracle SVGP) of a case"""
    likname, N, Dd, kind, scale, mode, mean = CASES[name]
    X, y, Z, idx = data(likname, N, Dd)
    lik = oracle_lik(R, likname)
    sc = scale if np.isscalar(scale) else np.asarray(scale, dtype=np.float64)
    ref = R.SVGP(R.Kernel(kind, sc, KVAR), lik, Z, stochastic=True, batchsize=min(B, N), elbo_mode=mode)
    if mean is not None:
        for gp in ref.latents:
            gp.mu0 = np.full(M, float(mean))
    ref.train(X, y, STEPS, idx_stream=idx)
    yt = R.treat_labels(y, lik)
    return X, y, yt, Z, idx, ref


def make_model(AGP, name, T=np.float64, **kw):
    """the host mirror's model of a case, trained on the case's index stream"""
    likname, N, Dd, kind, scale, mode, mean = CASES[name]
    X, y, Z, idx = data(likname, N, Dd)
    base = {"sqexponential": AGP.SqExponentialKernel, "matern52": AGP.Matern52Kernel}[kind]()
    tr = AGP.ScaleTransform(float(scale)) if np.isscalar(scale) else AGP.ARDTransform(np.asarray(scale, dtype=np.float64))
    model = AGP.SVGP(KVAR * (base @ tr), agp_lik(AGP, likname), AGP.AnalyticSVI(min(B, N)), Z, optimiser=False, mean=mean, T=T,
                     elbo_mode=mode, **kw)
    AGP.train_(model, X, y, STEPS, idx_stream=idx)
    return model


def restated_terms(ref, X, yt, chunk=CHUNK):
    """(data term, Gaussian KL, augmented KL) of ELBO(model, X, y) the way the streamed evaluation forms them: chunks of `chunk`
    points, predict_f(cov=True) moments, init_local_vars + local_updates per chunk, expec_loglikelihood and augmented_kl per chunk,
    gaussian_kl once.  The reference's once-per-evaluation terms (LogisticSoftMax log(beta[0]); the Laplace GIGEntropy's
    scalar-iteration terms in 'reference' mode) are what a chunk after the first must not count again: they are taken out of its
    augmented_kl."""
    lik = ref.likelihood
    e = akl = 0.0
    for s in range(0, len(X), chunk):
        xs, ys = X[s:s + chunk], yt[s:s + chunk]
        mu, var = ref.predict_f(xs, cov=True)
        lv = R.local_updates(R.init_local_vars(lik, len(xs)), lik, ys, mu, var)
        e += R.expec_loglikelihood(lik, ys, mu, var, lv, ref.elbo_mode)
        a = R.augmented_kl(lik, lv, ys, ref.elbo_mode)
        if s > 0:
            if lik.name == "logisticsoftmax":
                a -= math.log(lv["beta"][0])
            elif lik.name == "laplace" and ref.elbo_mode == "reference":
                sab0 = math.sqrt(lik.a * lv["b"][0] ** 2)
                a -= math.log(lik.a) / 2.0 + float(R.log2besselk_half(np.array([sab0]))[0])
        akl += a
    kl = sum(R.gaussian_kl(gp.mu, gp.mu0, gp.Sigma, gp.L) for gp in ref.latents)
    return float(e), float(kl), float(akl)

