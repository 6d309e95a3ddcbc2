"""CPU checks of the MOVGP restatement (tests/_movgp_ref.py), of the shared parity inputs (tests/_movgp_cases.py) and of the
constructor's refusals and defaults."""
import numpy as np
import pytest

import _movgp_cases as MC
from _movgp_ref import MOVGPRef
from _vgp_ref import VGPRef
from oracle import agp_ref as R


def _run(ref, yt, n):
    for _ in range(n):
        ref.step(yt)
    return ref


def test_one_latent_one_task_is_vgp():
    """Q = 1, one task, A = [[1]], Aoptimiser off: mu, Sigma and the ELBO are VGPRef's over 5 steps"""
    c = MC._case(("logistic",), 1, 60, False)
    X, ys, yt, A, mean, _ = MC.make_ref(c, R)
    a = MOVGPRef(R.Kernel("sqexponential", 2.0, 1.5), [R.LogisticLikelihood()], X, np.ones((1, 1)))
    b = VGPRef(R.Kernel("sqexponential", 2.0, 1.5), R.LogisticLikelihood(), X)
    for _ in range(5):
        a.step(yt)
        b.step(yt[0])
        assert np.max(np.abs(a.mu[0] - b.mu[0])) <= 1e-12 * np.max(np.abs(b.mu[0]))
        assert np.max(np.abs(a.Sigma[0] - b.Sigma[0])) <= 1e-12 * np.max(np.abs(b.Sigma[0]))
        assert abs(a.elbo(yt) - b.elbo(yt[0])) <= 1e-12 * abs(b.elbo(yt[0]))
    assert a.elbo_fresh(yt) == pytest.approx(b.elbo_fresh(yt[0]), rel=1e-12)


def test_agrees_with_mosvgp_z_equals_x():
    """Against the sparse oracle R.MOSVGP with Zs = [X] * Q, full batch, Aoptimiser off, 10 iterations on the bounded case Logistic +
    Laplace(2) + StudentT(3), Q = 2, N = 173: the two differ only through kappa = I - jitt K^-1.  The two CPU restatements give
    max_q max |mu_q - mu_q'| / max |mu_q| = 6.917e-3 on this input (ELBO -1251.56 against -1252.51); the bound is 3x that value."""
    c = MC._case(("logistic", "laplace", "studentt"), 2, 173, False)
    X, ys, yt, A, mean, ref = MC.make_ref(c, R)
    _run(ref, yt, 10)
    sv = R.MOSVGP(R.Kernel("sqexponential", 2.0, 1.5), ref.liks, [X.copy() for _ in range(2)], A.copy(), A_opt=None)
    sv.train(X, yt, 10)
    d = max(np.max(np.abs(ref.mu[q] - sv.latents[q].mu)) / np.max(np.abs(ref.mu[q])) for q in range(2))
    print("max rel mu difference", d)
    assert d < 3 * 6.917e-3
    assert np.array_equal(ref.A, A) and np.array_equal(sv.A, A)  # (Aoptimiser off: A stays)


@pytest.mark.parametrize("tasks,Q", [(("logistic", "laplace", "studentt"), 2), (("gaussian", "logistic"), 3),
                                     (("bsvm", "negbin"), 2)])
def test_grad_A_matches_finite_differences(tasks, Q):
    """update_A!'s gradient against central differences of sum_t E_q[log p_t] as a function of A, local variables and posterior
    fixed.  The function is quadratic in A, so the central difference is exact up to rounding: 1e-7 of the largest entry."""
    c = MC._case(tasks, Q, 60, False)
    X, ys, yt, A, mean, ref = MC.make_ref(c, R)
    _run(ref, yt, 2)
    g = ref.grad_A(yt)
    fd, h = np.zeros_like(g), 1e-5
    A0 = ref.A.copy()
    for t in range(ref.n_task):
        for q in range(Q):
            vals = []
            for s in (+h, -h):
                ref.A = A0.copy()
                ref.A[t, q] += s
                vals.append(ref.expec(yt))
            fd[t, q] = (vals[0] - vals[1]) / (2 * h)
    ref.A = A0
    assert np.max(np.abs(g - fd)) < 1e-7 * np.max(np.abs(g)), (g, fd)


def test_update_A_steps_uphill_and_keeps_the_rows_on_the_sphere():
    c = MC._case(("logistic", "laplace"), 3, 60, True)
    X, ys, yt, A, mean, ref = MC.make_ref(c, R, a_opt=None)
    _run(ref, yt, 2)
    ref.A_opt = R.Adam(0.01)  # (the optimiser's first step comes now)
    ref.A_state = [ref.A_opt.init(ref.A[t]) for t in range(ref.n_task)]
    A0, g = ref.A.copy(), ref.grad_A(yt)
    ref.update_A(yt)
    assert np.allclose(np.linalg.norm(ref.A, axis=1), 1.0, rtol=0, atol=1e-14)
    assert not np.array_equal(ref.A, A0)
    # ADAM's bias-corrected first step moves every weight by eta in the gradient's direction (ascent), before the projection
    want = A0 + 0.01 * np.sign(g)
    assert np.allclose(ref.A, want / np.linalg.norm(want, axis=1, keepdims=True), rtol=0, atol=1e-7)


@pytest.mark.parametrize("kernels", [[("sqexponential", 2.0, 1.5)],
                                     [("matern52", (1.3, 2.2, 0.7), 1.5), ("matern32", 1.4, 0.9)]])
def test_hyper_grad_matches_autograd(kernels):
    """the hyper gradient of every latent against torch autograd of -sum_q GaussianKL_q (only latent q's KL depends on kernel q)"""
    from _torch_elbo import neg_kl_hypergrad

    c = MC._case(("logistic", "laplace"), 2, 40, True, kernels=kernels, mean="empirical")
    X, ys, yt, A, mean, ref = MC.make_ref(c, R)
    _run(ref, yt, 3)
    for q in range(2):
        kind, scale, var = kernels[q % len(kernels)]
        dv, ds = ref.hyper_grad(q)
        av, as_ = neg_kl_hypergrad(kind, X, np.asarray(scale) if np.ndim(scale) else scale, var, ref.mu[q], ref.mu0[q],
                                   ref.Sigma[q])
        assert abs(dv - av) < 1e-10 * max(1.0, abs(av)), (dv, av)
        assert np.max(np.abs(ds - as_)) < 1e-10 * max(1.0, np.max(np.abs(as_))), (ds, as_)


def test_hyper_step_moves_every_latent_with_its_own_gradient():
    c = MC._case(("logistic", "laplace"), 2, 40, True)
    X, ys, yt, A, mean, ref = MC.make_ref(c, R)
    _run(ref, yt, 3)
    grads = [ref.hyper_grad(q) for q in range(2)]
    ref.hyper_step(R.Adam(0.01))
    for q in range(2):
        assert np.log(ref.kernels[q].sigma2 / 1.5) == pytest.approx(0.01 * np.sign(grads[q][0]), rel=1e-6)
        assert np.log(ref.kernels[q].scale / 2.0) == pytest.approx(0.01 * np.sign(np.sum(grads[q][1])), rel=1e-6)
    assert grads[0][0] != grads[1][0]


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_parity_inputs_stay_bounded(case):
    """the condition every parity input must satisfy (see _movgp_cases.py)"""
    X, ys, yt, A, mean, ref = MC.make_ref(case, R)
    _run(ref, yt, MC.ITERS)
    mm, cc = MC.bounded(ref)
    print(MC.case_id(case), "max |mu|", mm, "cond(-2 eta2)", cc)
    assert mm <= MC.MAX_MU and cc <= MC.MAX_COND


@pytest.mark.parametrize("name", sorted(MC.EXTRA))
def test_other_gpu_inputs_stay_bounded(name):
    """... and the inputs of the other GPU tests, after the iterations they are run for (hyper steps included where they take them)"""
    case, iters, hyper = MC.EXTRA[name]
    X, ys, yt, A, mean, ref = MC.make_ref(case, R)
    ref.train(yt, iters, opt=R.Adam(0.01) if hyper else None)
    mm, cc = MC.bounded(ref)
    print(name, MC.case_id(case), "max |mu|", mm, "cond(-2 eta2)", cc)
    assert mm <= MC.MAX_MU and cc <= MC.MAX_COND


def test_case_table_covers_what_it_must():
    ids = [MC.case_id(c) for c in MC.CASES]
    assert len(set(ids)) == len(ids)
    for tasks, Qs in MC.BOUNDED:
        for Q in Qs:
            for N in (173, 200):
                for aopt in (True, False):
                    assert any(c["tasks"] == tasks and c["Q"] == Q and c["N"] == N and c["aopt"] == aopt for c in MC.CASES)
    assert any(c["Q"] > len(c["tasks"]) for c in MC.CASES) and any(c["Q"] < len(c["tasks"]) for c in MC.CASES)
    assert any(len(c["kernels"]) == 2 for c in MC.CASES)
    assert {c["mean"] for c in MC.CASES} == {None, "constant", "empirical"}


def test_pinned_diverging_input():
    """Gaussian(0.05) + Logistic on Q = 3 latents, N = 60, Aoptimiser on: the restatement and the sparse oracle with Zs = [X] * Q both
    end, after 10 iterations, with an ELBO below 100 x their first one (both negative): the divergence is the reference's scheme"""
    c = MC.DIVERGING
    X, ys, yt, A, mean, ref = MC.make_ref(c, R)
    e = []
    for _ in range(10):
        ref.step(yt)
        e.append(ref.elbo(yt))
    sv = R.MOSVGP(R.Kernel("sqexponential", 2.0, 1.5), ref.liks, [X.copy() for _ in range(3)], A.copy(), A_opt=R.Adam(0.01))
    es = []
    sv.train(X, yt, 10, callback=lambda M, it, xb, yb: es.append(M.elbo(yb)))
    print("restatement", e[0], e[-1], "sparse oracle", es[0], es[-1], "max |mu|", MC.bounded(ref)[0])
    assert e[0] < 0 and es[0] < 0
    assert e[-1] < 100 * e[0] and es[-1] < 100 * es[0]
    assert MC.bounded(ref)[0] > MC.MAX_MU  # and it fails the parity condition, as it should


def test_constructor_refusals_and_defaults():
    import agp_amd as AGP

    rng = np.random.default_rng(0)
    X = rng.random((20, 2))
    ys = [(X[:, 0] > 0.5).astype(int), X[:, 1] + 0.1 * rng.standard_normal(20)]
    liks = lambda: [AGP.LogisticLikelihood(), AGP.LaplaceLikelihood(2.0)]  # noqa: E731
    k = AGP.SqExponentialKernel()
    with pytest.raises(TypeError, match="The inference object should be of type `AnalyticVI`"):
        AGP.MOVGP(X, ys, k, liks(), "not an inference", 2)
    with pytest.raises(ValueError, match="AnalyticVI"):
        AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticSVI(5), 2)
    with pytest.raises(NotImplementedError):
        AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 2, T=np.float32)
    with pytest.raises(ValueError, match="Number of kernels should be equal to the number of tasks"):
        AGP.MOVGP(X, ys, [k, k, k], liks(), AGP.AnalyticVI(), 2)
    with pytest.raises(ValueError, match="EmpiricalMean"):
        AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 2, mean=np.zeros(7))
    with pytest.raises(ValueError):
        AGP.MOVGP(X, [ys[0], ys[1][:10]], k, liks(), AGP.AnalyticVI(), 2)
    with pytest.raises(ValueError, match="A must be"):
        AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 2, A=np.eye(3))
    m = AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 3, optimiser=True, seed=1)
    assert m.k_opt.eta == 0.01 and m.A_opt.eta == 0.01  # MOVGP.jl:57,61,82-88
    assert AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 3).k_opt.eta == 0.01
    m0 = AGP.MOVGP(X, ys, k, liks(), AGP.AnalyticVI(), 3, optimiser=False, Aoptimiser=False)
    assert m0.k_opt is None and m0.A_opt is None and m0.z_opt is None
    assert AGP.n_latent(m) == 3 and m.n_task == 2 and m.m == m.N == 20 and m.T == np.dtype(np.float64)
    assert m.A.shape == (2, 3) and np.allclose(np.linalg.norm(m.A, axis=1), 1.0, rtol=0, atol=1e-14)  # rows of A normalised
    assert all(z.shape == (20, 2) and np.array_equal(z, X) for z in m.Zs)
    # one kernel: every latent owns a deep copy (kernels[mod1(i, 1)]); num_latent kernels: one each, in order
    assert len({id(q) for q in m.kernels}) == 3 and all(q is not k for q in m.kernels)
    k2 = [2.0 * (AGP.Matern52Kernel() @ AGP.ScaleTransform(1.5)), AGP.SqExponentialKernel(), 0.5 * AGP.Matern32Kernel()]
    m2 = AGP.MOVGP(X, ys, k2, liks(), AGP.AnalyticVI(), 3)
    assert [type(q).__name__ for q in m2.kernels] == ["Matern52Kernel", "SqExponentialKernel", "Matern32Kernel"]
    assert repr(m).startswith("Multioutput Variational Gaussian Process with the likelihoods ") and " infered by " in repr(m)
    assert m.X.shape == (20, 2) and AGP.MOVGP(X.T, ys, k, liks(), AGP.AnalyticVI(), 2, obsdim=2).X.shape == (20, 2)
