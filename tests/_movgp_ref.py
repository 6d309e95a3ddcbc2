"""NumPy restatement of the reference MOVGP with AnalyticVI (src/models/MOVGP.jl), on the oracle's likelihood pieces and on
tests/_vgp_ref.py for everything a latent does on its own (kernel matrices, Gaussian-KL hyper gradient, ADAM hyper step, train loop).

update_A  update_A! (single_and_multi_output_utils.jl:87-118) on mean_f_q = mu_q, var_f_q = diag Sigma_q of the current posterior and
          the local variables of the previous step: ADAM ascent, then every row of A back on the unit sphere
step      update_parameters!(::MOVGP) (training.jl:146-151): update_A, then per task the local update on the mixed
          (sum_q A_tq mu_q, sum_q A_tq^2 diag Sigma_q), the mixed gradients per latent (:48-84) -- each holds the OTHER latents
          fixed -- and natural_gradient!(::VarLatent) for all latents at once (analyticVI.jl:87-140)
elbo      analyticVI.jl:277-297: sum_t expec_loglikelihood_t - sum_q GaussianKL_q - sum_t AugmentedKL_t
predict   the multi-output _predict_f (predictions.jl:52-92) with Zviews(m) = X: means mixed by A, variances / covariances by A^2
hyper     the full-model method (autotuning.jl:48-84): only the Gaussian KL depends on a latent's kernel (VGPRef.hyper_grad)
"""
import copy

import numpy as np
import scipy.linalg as sla

from _vgp_ref import VGPRef
from oracle import agp_ref as R


class MOVGPRef(VGPRef):
    def __init__(self, kernels, liks, X, A, A_opt=None, jitter=1e-4, mu0=None):
        """kernels: one R.Kernel or Q of them; liks: one oracle likelihood per task; A: (n_task, Q); A_opt: R.Adam or None"""
        self.liks, self.X, self.jitter = list(liks), np.asarray(X, dtype=np.float64), jitter
        self.A = np.array(A, dtype=np.float64)
        self.n_task, self.nl = self.A.shape
        N = len(self.X)
        ks = list(kernels) if isinstance(kernels, (list, tuple)) else [kernels]
        self.kernels = [copy.deepcopy(ks[q % len(ks)]) for q in range(self.nl)]  # kernels[mod1(i, n_kernel)]  MOVGP.jl:99-101
        self.mu0 = [np.zeros(N) if mu0 is None else np.asarray(mu0, float).copy() for _ in range(self.nl)]
        self.mu = [np.zeros(N) for _ in range(self.nl)]
        self.Sigma = [np.eye(N) for _ in range(self.nl)]
        self.eta1 = [np.zeros(N) for _ in range(self.nl)]
        self.eta2 = [-0.5 * np.eye(N) for _ in range(self.nl)]
        self.lv = [R.init_local_vars_single(l, N) for l in self.liks]
        self.A_opt = A_opt
        self.A_state = [A_opt.init(self.A[t]) for t in range(self.n_task)] if A_opt else None
        self.refresh_K()

    def mixed(self):
        m, v = self.mean_f(), self.var_f()
        return ([sum(self.A[t, q] * m[q] for q in range(self.nl)) for t in range(self.n_task)],
                [sum(self.A[t, q] ** 2 * v[q] for q in range(self.nl)) for t in range(self.n_task)])

    def grad_A(self, ys):
        """d sum_t E_q[log p_t] / d A at fixed local variables and posterior, as update_A! writes it"""
        m, v = self.mean_f(), self.var_f()
        dA = np.zeros_like(self.A)
        for t, l in enumerate(self.liks):
            gmu = R.grad_E_mu(l, ys[t], self.lv[t])[0]
            gS = R.grad_E_Sigma(l, ys[t], self.lv[t])[0]
            for q in range(self.nl):
                others = sum(self.A[t, k] * m[k] for k in range(self.nl) if k != q)
                dA[t, q] = (np.dot(gmu, m[q]) - 2.0 * np.dot(gS, m[q] * others)
                            - 2.0 * self.A[t, q] * np.dot(gS, m[q] ** 2 + v[q]))
        return dA

    def update_A(self, ys):
        if self.A_opt is None:
            return
        dA = self.grad_A(ys)  # (row t of the gradient reads row t of A only: the rows may be stepped one after another)
        for t in range(self.n_task):
            self.A_state[t], d = self.A_opt.apply(self.A_state[t], dA[t])
            self.A[t] = self.A[t] + d
            self.A[t] = self.A[t] / np.sqrt(np.sum(self.A[t] ** 2))

    def step(self, ys):
        self.update_A(ys)
        m = self.mean_f()
        mt, vt = self.mixed()
        for t, l in enumerate(self.liks):
            self.lv[t] = R.local_updates(self.lv[t], l, ys[t], (mt[t],), (vt[t],))
        gmu = [R.grad_E_mu(l, ys[t], self.lv[t])[0] for t, l in enumerate(self.liks)]
        gS = [R.grad_E_Sigma(l, ys[t], self.lv[t])[0] for t, l in enumerate(self.liks)]
        for q in range(self.nl):
            g1 = sum(self.A[t, q] * (gmu[t] - 2.0 * gS[t] * (mt[t] - self.A[t, q] * m[q])) for t in range(self.n_task))
            g2 = sum(self.A[t, q] ** 2 * gS[t] for t in range(self.n_task))
            self.eta1[q] = g1 + sla.cho_solve((self.Ls[q], True), self.mu0[q])
            self.eta2[q] = -(np.diag(g2) + self.Kinvs[q] / 2.0)
        for q in range(self.nl):
            self.mu[q], self.Sigma[q] = R.natural_to_standard(self.eta1[q], self.eta2[q])
        return self

    def expec(self, ys, lv=None):
        """sum_t E_q[log p_t] on the mixed (mean_f, var_f)"""
        lv = self.lv if lv is None else lv
        mt, vt = self.mixed()
        return sum(R.expec_loglikelihood(l, ys[t], (mt[t],), (vt[t],), lv[t]) for t, l in enumerate(self.liks))

    def elbo(self, ys):
        kl = sum(R.gaussian_kl(self.mu[q], self.mu0[q], self.Sigma[q], self.Ls[q]) for q in range(self.nl))
        return float(self.expec(ys) - kl - sum(R.augmented_kl(l, self.lv[t], ys[t]) for t, l in enumerate(self.liks)))

    def elbo_fresh(self, ys):
        """ELBO(model) on the training set with fresh local variables (ELBO.jl:28-47)"""
        mt, vt = self.mixed()
        saved = self.lv
        self.lv = [R.local_updates(R.init_local_vars_single(l, len(self.X)), l, ys[t], (mt[t],), (vt[t],))
                   for t, l in enumerate(self.liks)]
        out = self.elbo(ys)
        self.lv = saved
        return out

    def predict_f(self, Xt):
        """per task (mean, variance, full covariance): the latents' predictions (VGPRef.predict_f) mixed by A / A^2"""
        mus, vars_, covs = VGPRef.predict_f(self, Xt)
        mix = lambda w, xs: [sum(w[t, q] * xs[q] for q in range(self.nl)) for t in range(self.n_task)]  # noqa: E731
        return mix(self.A, mus), mix(self.A ** 2, vars_), mix(self.A ** 2, covs)

    def predict_y(self, Xt):
        helper = R.MOSVGP.__new__(R.MOSVGP)
        helper.likelihoods = self.liks
        helper.predict_f = lambda Xq: tuple(self.predict_f(Xq)[0])
        return R.MOSVGP.predict_y(helper, Xt)

    def proba_y(self, Xt):
        mu, var, _ = self.predict_f(Xt)
        return [R.compute_proba(l, (mu[t],), (var[t],)) for t, l in enumerate(self.liks)]
