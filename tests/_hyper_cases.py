"""The hyper-gradient edge cases, shared by tests/test_hyper_edges_host.py (which checks on the CPU that the two references agree on
every case and that no gradient entry the device is compared on hides behind a larger one) and tests/test_gpu_hyper_edges.py
(which compares the device with both references on exactly these inputs).

What the cases reach (agp_hyper.h, kernel_backward_body): the backward pass through the kernel matrix stages KM_DC = 32 input
dimensions at a time.  D <= 32 is one chunk that pass 2 finds still staged; 32 < D <= 64 = HB_MAXD is two chunks that pass 2
stages again, with the row and column sums of the tile computed once; D > 64 is refused.  m and B off the 64-grid reach the guards
on G, the padded rows of the inducing-point partial sums and the number of row tiles the reductions add up.

The inputs keep the problem well conditioned at every D, because two independent references are compared at 1e-9 and the device
at 1e-7 / 1e-8:
* X uniform in [0, 1]^D, N = max(3 B, 200), three steps without optimiser, variance 1.3;
* D >= 2: base scale 3 / sqrt(D), which keeps the median squared scaled distance near 1.5 at every D; ARD cases multiply it per
  dimension by 0.7 + 0.6 u; Z is a random subset of X (coincident points in the K_nm pass: the truth for the default initialisation);
  the latent function depends on every dimension;
* D = 1: 65 random points of [0, 1] at scale 3 give cond(K) ~ 5e5 and the two references then differ by up to 2e-5 in dZ; Z on a
  jittered grid at scale 100 brings them to 1e-11;
* a kernel without transform has scale 1 by definition: at D = 33 / 64 the points then lie far apart (cond(K) ~ 20 / 2) and the
  gradients stay of order one, so these cases keep the same X.
"""
import functools

import numpy as np

VARIANCE = 1.3
ITERS = 3    # steps before a gradient is taken
STREAM = 5   # minibatches drawn per case: train_ takes its first hyper step after the fourth of five iterations
KERNELS = {"sqexponential": "SqExponentialKernel", "matern52": "Matern52Kernel", "matern32": "Matern32Kernel"}
KINDS = tuple(KERNELS)

# name -> (D, m, B): the smallest shapes at which each branch exists
SHAPES = {
    "d1": (1, 65, 63),        # one dimension, 31 padded staging columns; two column tiles of Z, one partial row tile
    "d31": (31, 63, 65),      # last dimension below the chunk edge; partial single tile of Z, two row tiles
    "d32": (32, 64, 64),      # exactly one full chunk, exactly one tile (the benchmark's D)
    "d33": (33, 130, 129),    # one dimension in the second chunk; three column tiles, three row tiles, both ragged
    "d64": (64, 130, 129),    # two full chunks (HB_MAXD)
    "d64f": (64, 192, 256),   # aligned, three block columns: a hyper step inside train_ takes the fused G_K (k_hyper_gK_fused)
}
GRAD_SHAPES = tuple(SHAPES)
SHAPES["d65"] = (65, 65, 63)  # above HB_MAXD: refused (refused_case below; in no table of gradient cases)
RAGGED2 = ("d33", "d64")      # the two-chunk ragged shapes that carry the crosses below
# likelihoods with a restatement in tests/_torch_elbo.py (autograd_hypergrad); the others are compared with the oracle only
RESTATED = ("logistic", "gaussian", "studentt")


def _case(shape, kind, transform="ard", lik="logistic", mode="corrected", f32=False, seed=0):
    D, m, B = SHAPES[shape]
    return dict(shape=shape, D=D, m=m, B=B, kind=kind, transform=transform, lik=lik, mode=mode, f32=f32, seed=seed)


def case_id(c):
    s = f"{c['shape']}-{c['kind']}-{c['transform']}-{c['lik']}"
    return s + ("-reference" if c["mode"] == "reference" else "") + ("-f32" if c["f32"] else "")


# every shape, every kernel kind, ARD, logistic
CASES = [_case(s, k) for s in GRAD_SHAPES for k in KINDS]
# ScaleTransform and no transform on the two-chunk ragged shapes
CASES += [_case("d33", "sqexponential", "scale"), _case("d33", "matern32", "none"),
          _case("d64", "matern52", "scale"), _case("d64", "sqexponential", "none")]
# Gaussian and StudentT on the same shapes
CASES += [_case("d33", "matern32", lik="gaussian"), _case("d33", "sqexponential", lik="studentt"),
          _case("d64", "sqexponential", lik="gaussian"), _case("d64", "matern52", lik="studentt")]
# k_hyper_gvec modes 1 (logistic, reference ELBO), 2 (BayesianSVM, reference ELBO), 3 (heteroscedastic: the two-product path with
# k_hyper_varf, two latents); LogisticSoftMax(3): several latents, one k_kernel_backward2 each
# (BayesianSVM: seeds 0 and 1 leave one column of dZ at 0.035 of the largest entry, below the floor of
#  tests/test_hyper_edges_host.py; seed 4 has 0.11)
CASES += [_case("d33", "matern52", mode="reference"), _case("d64", "sqexponential", lik="bayesiansvm", mode="reference", seed=4),
          _case("d33", "sqexponential", lik="heteroscedastic"), _case("d64", "matern32", lik="logisticsoftmax")]
F32_CASES = [_case(s, k, f32=True) for s in RAGGED2 for k in ("sqexponential", "matern52")]

# the full model (kernel_grad: X on both sides, k_vgp_gK, no dZ): (D, N, kind, transform)
VGP_CASES = [(1, 65, "sqexponential", "scale"), (32, 130, "matern52", "ard"), (33, 65, "matern32", "ard"),
             (33, 130, "sqexponential", "ard"), (64, 65, "sqexponential", "scale"), (64, 130, "matern52", "ard")]


def refused_case():
    """D = 65, one dimension above HB_MAXD, on the same recipe"""
    return _case("d65", "sqexponential")


def scales_of(c, rng):
    D = c["D"]
    base = 100.0 if D == 1 else 3.0 / np.sqrt(D)
    if c["transform"] == "ard":
        return base * (0.7 + 0.6 * rng.random(D))
    return base if c["transform"] == "scale" else 1.0


@functools.lru_cache(maxsize=None)
def _inputs(shape, transform, lik, seed):
    D, m, B = SHAPES[shape]
    rng = np.random.default_rng(1000 * D + m + seed)
    N = max(3 * B, 200)
    X = rng.random((N, D))
    w = rng.standard_normal(D)
    f = 1.5 * np.sin(3.0 * X @ w / np.sqrt(D)) + X[:, 0] - 0.5
    if D == 1:
        Z = ((np.arange(m) + 0.5 + 0.3 * (rng.random(m) - 0.5)) / m)[:, None]
    else:
        Z = X[rng.permutation(N)[:m]].copy()
    sc = scales_of(dict(D=D, transform=transform), rng)
    if lik in RESTATED:
        y = {"logistic": lambda: (f + 0.3 * rng.standard_normal(N) > 0).astype(np.int64),
             "gaussian": lambda: f + 0.2 * rng.standard_normal(N),
             "studentt": lambda: f + 0.2 * rng.standard_t(3, N)}[lik]()
    else:
        from _liks import labels

        y = labels(lik, f, X, rng)
    idx = [rng.choice(N, B, replace=False) for _ in range(STREAM)]
    for a in (X, Z, y, *idx):
        a.setflags(write=False)
    return X, y, Z, sc, idx


def make_inputs(c):
    """(X, y, Z, scales, idx stream of STREAM minibatches) of a case: read-only arrays, the same objects on every call.  scales: D
    numbers (ARD), one number (ScaleTransform) or 1.0 (no transform).  An f32 case has the inputs of its f64 twin."""
    return _inputs(c["shape"], c["transform"], c["lik"], c["seed"])


def oracle_lik(R, c):
    if c["lik"] == "gaussian":
        return R.GaussianLikelihood(0.05)
    if c["lik"] == "studentt":
        return R.StudentTLikelihood(3.0, 0.5)
    from _liks import oracle_lik as tab

    return tab(R, c["lik"])


def device_lik(AGP, c):
    if c["lik"] == "gaussian":
        return AGP.GaussianLikelihood(0.05)
    if c["lik"] == "studentt":
        return AGP.StudentTLikelihood(3.0, 0.5)
    from _liks import agp_lik as tab

    return tab(AGP, c["lik"])


def device_kernel(AGP, kind, transform, sc):
    k = getattr(AGP, KERNELS[kind])()
    if transform != "none":
        k = k @ (AGP.ARDTransform(np.asarray(sc, dtype=np.float64)) if transform == "ard" else AGP.ScaleTransform(float(sc)))
    return VARIANCE * k


_ORACLE = {}


def oracle_run(c, R, iters=ITERS):
    """The oracle trained `iters` steps on the case's index stream, its kernel matrices refreshed on the last of these minibatches
    -> (model, xb, yb (treated), rho, [R.hyper_gradient per latent]).  Computed once per case and shared: nobody writes to it.
    An f32 case runs the oracle in float64 with the reference's Float32 jitter 1e-3."""
    key = (case_id(c), iters)
    if key not in _ORACLE:
        X, y, Z, sc, idx = make_inputs(c)
        lik = oracle_lik(R, c)
        ker = R.Kernel(c["kind"], np.array(sc, dtype=np.float64) if np.ndim(sc) else float(sc), VARIANCE,
                       has_transform=c["transform"] != "none")
        M = R.SVGP(ker, lik, np.array(Z), stochastic=True, batchsize=c["B"], elbo_mode=c["mode"],
                   jitter=1e-3 if c["f32"] else 1e-4)
        yt = R.treat_labels(np.array(y), lik)
        M.train(np.array(X), yt, iters, idx_stream=idx[:iters], labels_treated=True)
        xb, yb = np.array(X[idx[iters - 1]]), yt[idx[iters - 1]]
        M.hp_updated = True
        M.compute_kernel_matrices(xb)
        rho = len(X) / c["B"]
        _ORACLE[key] = (M, xb, yb, rho, [R.hyper_gradient(M, xb, yb, k, rho) for k in range(len(M.latents))])
    return _ORACLE[key]


def restated_lik(c):
    """the (name, params) tuple tests/_torch_elbo.py takes"""
    return (c["lik"], 0.05) if c["lik"] == "gaussian" else (c["lik"],)


def max_error(got, ref):
    """largest entry of |got - ref| relative to the largest entry of |ref|; inf when `got` holds anything that is not finite (a NaN
    must fail a comparison, and neither max() nor `<` can be trusted with one)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def errors(got, ref):
    """(dvariance error relative to max(1, |.|), dscale and dZ errors per entry relative to the vector's largest reference entry);
    got / ref: (dvariance, dscale[D], dZ[m, D]); inf for anything not finite"""
    ev = abs(got[0] - ref[0]) / max(1.0, abs(ref[0])) if np.isfinite(got[0]) else float("inf")
    return float(ev), max_error(got[1], ref[1]), max_error(got[2], ref[2])


def within(e, tol):
    """every figure of errors() below tol (a NaN is not)"""
    return all(bool(v < tol) for v in e)


def vgp_inputs(D, N, transform):
    """(X, y in {0, 1}, scales) of a full-model case, by the recipe above (D = 1: X itself on the jittered grid at scale 100)"""
    rng = np.random.default_rng(7000 + 100 * D + N)
    X = rng.random((N, D))
    if D == 1:
        X = ((np.arange(N) + 0.5 + 0.3 * (rng.random(N) - 0.5)) / N)[:, None]
    w = rng.standard_normal(D)
    f = 1.5 * np.sin(3.0 * X @ w / np.sqrt(D)) + X[:, 0] - 0.5
    y = (f + 0.3 * rng.standard_normal(N) > 0).astype(np.int64)
    return X, y, scales_of(dict(D=D, transform=transform), rng)
