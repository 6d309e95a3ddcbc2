"""The inputs of the class-count tests, shared by the CPU suite (tests/test_multiclass_cases_host.py, which recomputes from the
constants in the headers what every case claims to reach) and the GPU suite (tests/test_gpu_multiclass_counts.py).

The number of latents K of a multi-class model decides which instantiation of a kernel runs, how many launches a step takes and
which lanes sit idle inside a shuffle.  The tables below name, per K, the seam the case is there for; a changed constant in csrc/
makes the host test fail and forces a new choice of K.

Not reachable at test size and left untested: a task-graph chunk of ONE latent inside a multi-latent handle needs dag_nb = 1, i.e.
m >= 1024 with B >= 8128 (DAG_MAX_COLUMN_TILES / (nt + ne + 1) < 2)."""
import functools

import numpy as np

from oracle import agp_ref as R

TILE = 64

# ---- a. analytic LogisticSoftMax SVGP: m = 70 (mp = 128), D = 3, N = 400, AnalyticSVI(150), 4 steps on a fixed index stream --------
ANALYTIC = dict(m=70, D=3, N=400, B=150, steps=4, scale=3.0, variance=1.5, n_test=37)
# K -> lg: lanes per point of k_lsm_fused (None: the five-launch fallback); dag: chunks of augmented factorisations per task-graph
# launch; plain: chunks under AGP_CHOL_DAG=0 (a chunk of 1 is the single-problem potrf_fused branch); rowstats: k_rowstats_local
# launches; eta_batched: k_syrk_eta_batch takes the eta step of all latents in one launch
ANALYTIC_CASES = {
    2: dict(lg=2, dag=(2,), plain=(2,), rowstats=(2,), eta_batched=True),            # LG = 2, never launched before
    5: dict(lg=8, dag=(5,), plain=(5,), rowstats=(5,), eta_batched=True),            # LG = 8 with three idle lanes per point
    9: dict(lg=16, dag=(5, 4), plain=(9,), rowstats=(9,), eta_batched=True),         # LG = 16, seven idle lanes; unequal chunks
    10: dict(lg=16, dag=(5, 5), plain=(10,), rowstats=(10,), eta_batched=True),      # the ordinary ten-class model
    16: dict(lg=16, dag=(8, 8), plain=(16,), rowstats=(16,), eta_batched=True),      # every batched launch exactly full
    17: dict(lg=None, dag=(6, 6, 5), plain=(16, 1), rowstats=(16, 1), eta_batched=False),  # the first count past all of them
}
NO_TASK_GRAPH_KS = (16, 17)  # run again in a child under AGP_CHOL_DAG=0: a full CholBatch, and 16 + the lone seventeenth latent


def quantile_classes(f, K):
    """1-based classes from the K-quantiles of a score (tests/test_gpu_round3.py, test_many_classes_beyond_the_batched_launch_limits)"""
    return 1 + np.digitize(f, np.quantile(f, np.linspace(0, 1, K + 1)[1:-1]))


def analytic_data(K):
    c = ANALYTIC
    rng = np.random.default_rng(100 + K)
    X = rng.random((c["N"], c["D"]))
    f = np.sin(5 * X[:, 0]) + X[:, 1] * X[:, 2]
    y = quantile_classes(f, K)
    Z = X[rng.permutation(c["N"])[:c["m"]]].copy()
    idx = [rng.choice(c["N"], c["B"], replace=False) for _ in range(c["steps"])]
    Xt = rng.random((c["n_test"], c["D"]))
    return X, y, Z, idx, Xt


def oracle_kernel(scale=None):
    return R.Kernel("sqexponential", ANALYTIC["scale"] if scale is None else scale, ANALYTIC["variance"])


@functools.lru_cache(maxsize=None)
def analytic_oracle(K):
    """the oracle after ANALYTIC['steps'] steps and its ELBO after every step (computed once, left unchanged)"""
    X, y, Z, idx, Xt = analytic_data(K)
    mr = R.SVGP(oracle_kernel(), R.LogisticSoftMaxLikelihood(K), Z, stochastic=True, batchsize=ANALYTIC["B"])
    elbos = []
    mr.train(X, y, ANALYTIC["steps"], idx_stream=idx, callback=lambda M, it, xb, yb: elbos.append(M.elbo(yb)))
    mf, vf = mr.predict_f(Xt, cov=True)
    return dict(model=mr, elbo=elbos, mean=np.stack(mf), var=np.stack(vf), proba=mr.proba_y(Xt))


# ---- c. related cases at K = 10 ------------------------------------------------------------------------------------------------------
VGP10 = dict(K=10, N=65, D=3, steps=3, seed=5, scale=2.0, variance=1.5)  # N = 65: two tiles, 5 + 5 full-model factorisations
# On the data of ANALYTIC_CASES[10].  The training loop takes its first hyper step after the fourth iteration (n_iter >= 3,
# training.jl:65-69) and none after the last: six iterations are three plain ones, two hyper steps (after the fourth and the fifth)
# and two iterations whose ten kernels and inducing sets differ from latent to latent.  Three iterations would take no hyper step.
HYPER10 = dict(K=10, steps=6, k_eta=0.05, z_eta=0.01)


def vgp10_data():
    c = VGP10
    rng = np.random.default_rng(c["seed"])
    X = rng.random((c["N"], c["D"]))
    f = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.7
    return X, quantile_classes(f, c["K"])


def hyper10_data():
    X, y, Z, _, _ = analytic_data(HYPER10["K"])
    rng = np.random.default_rng(1010)
    return X, y, Z, [rng.choice(ANALYTIC["N"], ANALYTIC["B"], replace=False) for _ in range(HYPER10["steps"])]


@functools.lru_cache(maxsize=None)
def hyper10_oracle():
    X, y, Z, idx = hyper10_data()
    mr = R.SVGP(oracle_kernel(), R.LogisticSoftMaxLikelihood(HYPER10["K"]), Z, stochastic=True, batchsize=ANALYTIC["B"],
                k_opt=R.Adam(HYPER10["k_eta"]), z_opt=R.Adam(HYPER10["z_eta"]))
    mr.train(X, y, HYPER10["steps"], idx_stream=idx)
    return mr


# ---- d. the Monte-Carlo expectation kernel point by point ------------------------------------------------------------------------------
# K -> P: lanes per draw (the power of two >= K); G = 64 / P draws at a time; TS = MC_TILE / K draws per LDS tile
MC_POINT_CASES = {
    4: dict(P=4, G=16, TS=512),
    5: dict(P=8, G=8, TS=409),      # idle lanes at P = 8
    9: dict(P=16, G=4, TS=227),     # P = 16 with idle lanes
    16: dict(P=16, G=4, TS=128),    # P = 16, full
    17: dict(P=32, G=2, TS=120),    # P = 32, fifteen idle lanes: one cross-group butterfly stage
    32: dict(P=32, G=2, TS=64),
    33: dict(P=64, G=1, TS=62),     # P = 64: the group mask is all ones, no cross-group butterfly
    64: dict(P=64, G=1, TS=32),     # MC_KMAX
}
MC_POINTS = 41  # ten full workgroups of four waves and one with a single wave
MC_TRAJECTORY_KS = {10: dict(P=16, G=4, TS=204), 17: dict(P=32, G=2, TS=120)}  # the cases added to tests/_mcvi_cases.py


def mc_nmc(K):
    """one draw, a full tile, a tile and one draw, several tiles"""
    ts = MC_POINT_CASES[K]["TS"]
    return (1, ts, ts + 1, 1000)


def mc_point_inputs(K):
    """(c, mu, var) of _mcvi_cases.point_inputs(K, P=41) with three engineered points at var = 0 (f = mu exactly, for every draw):
    point 6: all K means equal, scored for class 0 -- the K-way tie, whose first maximum is class 0; point 7: the same, scored for
    class K - 1; point 8: the last two classes tie at the top, scored for the last"""
    import _mcvi_cases as CS

    c, mu, var = CS.point_inputs(K, P=MC_POINTS)
    mu[:, 6:8], var[:, 6:9] = 1.25, 0.0
    c[6], c[7] = 0, K - 1
    mu[:, 8] = np.linspace(-3.0, 0.5, K)
    mu[K - 2, 8] = mu[K - 1, 8] = 2.0
    c[8] = K - 1
    return c, mu, var


# ---- f. the log predictive density's multi-class branch ---------------------------------------------------------------------------------
LPD_KS = (2, 10, 17)
LPD_POINTS = 64


def lpd_inputs(K):
    """(c, mu, var): means in +-30, and in every point one class at +800 or -800"""
    rng = np.random.default_rng(900 + K)
    n = LPD_POINTS
    mu = rng.uniform(-30, 30, (K, n))
    far = rng.integers(0, K, n)
    mu[far, np.arange(n)] = np.where(np.arange(n) % 2 == 0, 800.0, -800.0)
    var = 10.0 ** rng.uniform(-12, 2, (K, n))
    c = rng.integers(0, K, n).astype(np.int32)
    c[:8] = far[:8]  # (scored for the far class itself: log p = 0 to rounding at +800, about -800 at -800)
    return c, mu, var


# ---- g. MOSVGP with MO_MAXT tasks -------------------------------------------------------------------------------------------------------
MO16 = dict(T=16, Q=5, m=24, N=300, D=2, B=100, steps=3, scale=3.0)
MO_KINDS = ("gaussian", "logistic", "studentt", "laplace")


def mo16_data():
    c = MO16
    rng = np.random.default_rng(1616)
    X = rng.random((c["N"], c["D"]))
    ys, kinds = [], []
    for t in range(c["T"]):
        f = np.sin((2.0 + 0.3 * t) * X[:, 0] + 0.4 * t) + (0.5 - 0.05 * t) * X[:, 1]
        kind = MO_KINDS[t % len(MO_KINDS)]
        kinds.append(kind)
        ys.append({"gaussian": lambda: f + 0.1 * rng.standard_normal(c["N"]),
                   "logistic": lambda: np.where(f - np.median(f) + 0.1 * rng.standard_normal(c["N"]) > 0, 1.0, -1.0),
                   "studentt": lambda: f + 0.1 * rng.standard_t(3, c["N"]),
                   "laplace": lambda: f + rng.laplace(0, 0.3, c["N"])}[kind]())
    A = rng.standard_normal((c["T"], c["Q"]))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Zs = [X[rng.permutation(c["N"])[:c["m"]]].copy() for _ in range(c["Q"])]
    idx = [rng.choice(c["N"], c["B"], replace=False) for _ in range(c["steps"])]
    Xt = rng.random((37, c["D"]))
    return X, ys, kinds, A, Zs, idx, Xt


def mo_oracle_lik(kind):
    return {"gaussian": lambda: R.GaussianLikelihood(0.05), "logistic": R.LogisticLikelihood,
            "studentt": lambda: R.StudentTLikelihood(3.0), "laplace": lambda: R.LaplaceLikelihood(0.3)}[kind]()


@functools.lru_cache(maxsize=None)
def mo16_oracle():
    X, ys, kinds, A, Zs, idx, Xt = mo16_data()
    mr = R.MOSVGP(R.Kernel("sqexponential", MO16["scale"], 1.0), [mo_oracle_lik(k) for k in kinds], Zs, A.copy(), stochastic=True,
                  batchsize=MO16["B"], A_opt=None)
    elbos = []
    mr.train(X, ys, MO16["steps"], idx_stream=idx, callback=lambda M, it, xb, yb: elbos.append(M.elbo(yb)))
    mf, vf = mr.predict_f(Xt, cov=True)
    return dict(model=mr, elbo=elbos, mean=np.stack(mf), var=np.stack(vf))
