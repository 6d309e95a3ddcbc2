"""CPU tests of the acquisition kinds that are evaluated in logarithms, LogEI and LogPI (include/agp_hip.h, "ACQUISITION FUNCTIONS";
csrc/agp_acq_log.h): the restatement tests/_acq_log_ref.py against mpmath at 100 digits, the two branches of the formulation against
each other at the branch point, the COMPILED point function -- csrc/agp_acq_log.h built for the host into tests/c_host/acq_log_point.cpp,
a program of its own -- against mpmath and against the restatement, the limits, exp(log alpha) against the plain kinds, the
conditioning of the plateau case that the GPU suite runs, and the host mirror.

The measure: |got - want| <= PARITY max(1, |want|) for log alpha, |got - want| <= PARITY |want| for its derivatives in mu and sigma.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _acq_log_ref as LR
import _acq_ref as A
from test_acq_host import grid_moments as plain_grid_moments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgaussianprocesses.jl_amd", "csrc")
PARITY = A.PARITY
EPS = float(np.finfo(np.float64).eps)


def assert_point(got, want, what):
    """got = (log alpha, d / d mu, d / d sigma) against the judge's, in the measure; prints the worst of each"""
    ea, em, es = LR.err_alpha(got[0], want[0]), LR.err_rel(got[1], want[1]), LR.err_rel(got[2], want[2])
    print(f"{what}: worst error log alpha {ea.max():.2e}  d/dmu {em.max():.2e}  d/dsigma {es.max():.2e}")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2])), what
    assert ea.max() <= PARITY and em.max() <= PARITY and es.max() <= PARITY, (what, int(np.argmax(ea)), int(np.argmax(em)), int(np.argmax(es)))
    return ea.max(), em.max(), es.max()


# ---- the restatement against mpmath ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_restatement_against_mpmath(kind, minimize):
    s = -1.0 if minimize else 1.0
    mu, var = LR.grid_moments(s)
    al, dm, ds, dv = LR.point(LR.acq(kind, minimize=minimize), mu, var)
    want = LR.mp_grid(kind, s)
    assert_point((al, dm, ds), want, f"{kind} s={s:+.0f}")
    assert_point((al, dm, dv * 2 * np.sqrt(var)), want, f"{kind} s={s:+.0f} (d/dvar 2 sigma)")
    al_ld, dm_ld, ds_ld, _ = LR.point(LR.acq(kind, minimize=minimize), mu, var, dtype=np.longdouble)
    assert_point((al_ld, dm_ld, ds_ld), want, f"{kind} s={s:+.0f} long double")


def test_the_grid_is_the_one_that_was_asked_for():
    z = set(LR.ZS)
    assert z >= {8.0, 1.0, 0.0, -0.5, -1.0, -3.0, -5.0, -12.0, -37.0, -38.0, -40.0, -100.0, -1e3, -1e6, -1e9} and len(z) == 17
    assert np.nextafter(-3.0, 0.0) in z and np.nextafter(-3.0, -4.0) in z and LR.SIGMAS == (1e-8, 1.0, 1e4)
    assert LR.BRANCH == -3.0 and LR.CF_TERMS == ((5.0, 60), (12.0, 32), (np.inf, 12))
    h = open(os.path.join(CSRC, "agp_acq_log.h")).read()  # the restatement's constants are the header's
    assert re.search(r"ACQ_LOG_BRANCH\s*=\s*-3\.0\s*;", h)
    assert re.search(r"return\s+t\s*<\s*5\.0\s*\?\s*60\s*:\s*\(\s*t\s*<\s*12\.0\s*\?\s*32\s*:\s*12\s*\)\s*;", h)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_incumbent_and_margin(kind):
    """best and xi off zero, both directions, moments that put z on both sides of the branch point"""
    rng = np.random.default_rng(7)
    mu, var = rng.normal(0.4, 1.0, 120), rng.uniform(0.01, 2.0, 120)
    var[:40] *= 1e-3  # z down to about -100
    for minimize in (False, True):
        q = LR.acq(kind, best=2.1 * q_sign(minimize), xi=0.05, minimize=minimize)
        got = LR.point(q, mu, var)
        want = np.array([LR.mp_point(kind, q["s"], q["best"], q["xi"], m, v) for m, v in zip(mu, var)]).T
        z = (q["s"] * (mu - q["best"]) - q["xi"]) / np.sqrt(var)
        assert np.any(z > LR.BRANCH) and np.any(z < LR.BRANCH)
        assert_point(got[:3], want, f"{kind} minimize={minimize}")


def q_sign(minimize):
    return -1.0 if minimize else 1.0


def test_the_cut_of_the_continued_fraction_by_range():
    """Fewer terms at larger t: in every range the cut must stay invisible in float64.  In long double, the fraction cut where the
    header cuts it against the fraction cut after 120: below eps / 8 of c at the lower end of every range (t = 3, 5, 12), at the
    neighbours of the two thresholds, and on t = 3 ... 50 in steps of 1 / 16; and one range further down it is NOT (the ranges are
    not wider than they may be)."""
    T = np.longdouble
    ends = [3.0, 5.0, 12.0, np.nextafter(5.0, 0.0), np.nextafter(12.0, 0.0)]
    t = np.concatenate([ends, np.arange(3.0, 50.0, 1.0 / 16.0)]).astype(T)
    full = LR.continued_fraction(t, 120)
    err = np.abs(LR.continued_fraction(t) - full) / full
    print(f"the cut by range: worst {float(err.max()):.2e} of c, at t = {float(t[np.argmax(err)])}")
    assert float(err.max()) <= EPS / 8
    for t0, fewer in ((3.0, 32), (5.0, 12)):  # the next range's count at this range's lower end
        e = float(abs(LR.continued_fraction(np.array([t0], dtype=T), fewer)[0] - LR.continued_fraction(np.array([t0], dtype=T), 120)[0]))
        assert e / float(LR.continued_fraction(np.array([t0], dtype=T), 120)[0]) > EPS / 8
    # and in float64 the three counts give the very bits of 60 terms wherever they apply, on the same points
    t64 = t.astype(np.float64)
    same = LR.continued_fraction(t64) == LR.continued_fraction(t64, 60)
    print(f"float64: {int(same.sum())} of {len(same)} values of c have the bits of the 60-term fraction")
    assert np.max(np.abs(LR.continued_fraction(t64) - LR.continued_fraction(t64, 60)) / LR.continued_fraction(t64, 60)) <= EPS


@pytest.mark.parametrize("kind", LR.KINDS)
def test_restatement_on_the_fine_grid_of_the_tail(kind):
    """z in [-12, -3] in steps of 0.05 and z = -20, -38, -50, -1e2, -1e3, -1e4, -1e6, -1e8 (where the term counts were measured), and
    the neighbours of the thresholds t = 5 and t = 12"""
    z = np.concatenate([np.arange(-12.0, -3.0 + 1e-9, 0.05), [-20.0, -38.0, -50.0, -1e2, -1e3, -1e4, -1e6, -1e8],
                        [np.nextafter(-5.0, 0.0), np.nextafter(-5.0, -9.0), np.nextafter(-12.0, 0.0), np.nextafter(-12.0, -20.0)]])
    z = z[z <= LR.BRANCH]
    got = LR.point(LR.acq(kind), z, np.ones_like(z))
    want = np.array([LR.mp_point(kind, 1.0, 0.0, 0.0, m, 1.0) for m in z]).T
    assert_point(got[:3], want, f"{kind} on the fine grid of the tail")


# ---- the branch point ---------------------------------------------------------------------------------------------------------------------
def _floats_around_the_branch():
    lo = [LR.BRANCH]
    for _ in range(500):
        lo.append(np.nextafter(lo[-1], -np.inf))
    hi = [LR.BRANCH]
    for _ in range(499):
        hi.append(np.nextafter(hi[-1], np.inf))
    z = np.array(lo[:0:-1] + hi)
    assert len(z) == 1000 and np.all(np.diff(z) > 0) and z[500] == LR.BRANCH
    return z


@pytest.mark.parametrize("kind", LR.KINDS)
def test_the_two_sides_of_the_branch_point(kind):
    """1000 consecutive floats z, 501 on the continued fraction's side (z <= -3) and 499 on the direct side; sigma = 1, best = xi = 0,
    so that mu IS z.  Both formulations on all of them agree within the measure.  Across the branch point the outputs are monotone:
    in exact arithmetic log alpha rises with z and both derivatives (Phi / h and phi / h; phi / Phi and -z phi / Phi) fall.  Neighbouring
    floats differ by 4.4e-16, the outputs by 1 to 2 units of their last place, so "monotone" can only be asked up to the rounding of
    the expressions themselves, and that bound is written down here from the number format, not taken from the code: on the direct
    side h = phi + z Phi keeps 1 / 11.7 of phi at z = -3 (phi = 4.43e-3, z Phi = -4.05e-3); the argument of erfc is a rounded product,
    which moves erfc(x) by x erfc'(x) / erfc(x) eps = 10 eps at x = 3 / sqrt 2; erfc itself is allowed 4 eps, the product z Phi and exp
    1 eps each: (10 + 4 + 1) 10.7 + 2 11.7 = 184 eps relative in h, and Phi / h, phi / h, log h inherit it.  No step may go against the
    direction by more than 256 eps = 5.7e-14, relative to the value (relative to max(1, |log alpha|) for log alpha): a step of the
    size of a formulation error at the branch point (1e-10 with 20 terms in the continued fraction) fails by three orders.  On the
    continued fraction's side, where nothing cancels, the sequence is monotone outright."""
    z = _floats_around_the_branch()
    one = np.ones_like(z)
    q = LR.acq(kind)
    cf = LR.point(q, z, one, branch=np.inf)[:3]
    direct = LR.point(q, z, one, branch=-np.inf)[:3]
    e = (LR.err_alpha(cf[0], direct[0]).max(), LR.err_rel(cf[1], direct[1]).max(), LR.err_rel(cf[2], direct[2]).max())
    print(f"{kind}: the two formulations on 1000 floats around z = -3: log alpha {e[0]:.2e}  d/dmu {e[1]:.2e}  d/dsigma {e[2]:.2e}")
    assert max(e) <= PARITY
    got = LR.point(q, z, one)[:3]
    assert all(np.array_equal(g[:501], c[:501]) and np.array_equal(g[501:], d[501:]) for g, c, d in zip(got, cf, direct))
    tol = 256 * EPS
    for name, o, direction in (("log alpha", got[0], 1.0), ("d/dmu", got[1], -1.0), ("d/dsigma", got[2], -1.0)):
        step = direction * np.diff(o)
        scale = np.maximum(1.0, np.abs(o[:-1])) if name == "log alpha" else np.abs(o[:-1])
        back = np.max(-step / scale)
        print(f"{kind} {name}: the largest step against the direction {max(back, 0.0):.2e} of the value; at the branch point {step[500] / scale[500]:+.2e}")
        assert direction * (o[-1] - o[0]) > 0, (kind, name)
        assert back <= tol, (kind, name, back)
        assert np.all(step[:500] >= 0), (kind, name)  # the continued fraction's side


# ---- the compiled point function ----------------------------------------------------------------------------------------------------------
def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """csrc/agp_acq_log.h compiled for the host into a program of its own (no sanitizer, nothing loaded into Python)"""
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path_factory.mktemp("acq_log") / "acq_log_point"
    cmd = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "c_host", "acq_log_point.cpp"), "-o", str(exe),
           "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(kind, s, best, xi, mu, var):
        """(log alpha, d / d mu, d / d var) of the moments, through hex floats: the program's bits"""
        lines = "".join(f"{LR.CODES[kind]} {float(s).hex()} {float(best).hex()} {float(xi).hex()} {float(m).hex()} {float(v).hex()}\n"
                        for m, v in zip(np.atleast_1d(mu), np.atleast_1d(var)))
        out = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, check=True).stdout.split()
        return np.array([float.fromhex(t) for t in out]).reshape(-1, 3).T

    return run


@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_compiled_point_function(program, kind, minimize):
    s = -1.0 if minimize else 1.0
    mu, var = LR.grid_moments(s)
    al, dm, dv = program(kind, s, 0.0, 0.0, mu, var)
    sg2 = 2 * np.sqrt(var)
    assert_point((al, dm, dv * sg2), LR.mp_grid(kind, s), f"compiled {kind} s={s:+.0f} against mpmath")
    ref = LR.point(LR.acq(kind, minimize=minimize), mu, var)
    assert_point((al, dm, dv * sg2), (ref[0], ref[1], ref[3] * sg2), f"compiled {kind} s={s:+.0f} against the restatement")


def _limit_cases():
    """(mu, var) with best = 0.5, xi = 0: var in {0, -1e-12} with imp < 0, = 0, > 0 (by one unit of the last place too)"""
    mu = np.array([-1.0, 0.5, np.nextafter(0.5, 1.0), 2.0])
    return [(mu, np.full(4, v)) for v in (0.0, -1e-12)]


def _limits_want(kind, s, mu):
    imp = s * (mu - 0.5)
    up = imp > 0
    with np.errstate(all="ignore"):
        if kind == "logei":
            return np.where(up, np.log(np.where(up, imp, 1.0)), -np.inf), np.where(up, s / np.where(up, imp, 1.0), 0.0)
    return np.where(up, 0.0, -np.inf), np.zeros(4)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_limits_and_nan(kind, program):
    for minimize in (False, True):
        s = -1.0 if minimize else 1.0
        q = LR.acq(kind, best=0.5, minimize=minimize)
        for mu, var in _limit_cases():
            wa, wm = _limits_want(kind, s, mu)
            assert np.isneginf(wa).sum() >= 1 and np.isfinite(wa).sum() >= 1  # both sides of imp = 0 are there
            al, dm, ds, dv = LR.point(q, mu, var)
            assert np.array_equal(al, wa) and np.array_equal(dm, wm) and np.all(ds == 0) and np.all(dv == 0)
            cl, cm, cv = program(kind, s, 0.5, 0.0, mu, var)
            assert np.array_equal(cm, wm) and np.all(cv == 0) and np.array_equal(np.isneginf(cl), np.isneginf(wa))
            fin = np.isfinite(wa)
            assert np.all(np.abs(cl[fin] - wa[fin]) <= 2 * EPS * np.abs(wa[fin]))  # (log of the C library against NumPy's)
        for mu_, var_ in ((np.nan, 1.0), (0.3, np.nan), (np.nan, 0.0), (np.nan, np.nan), (np.nan, -1.0)):
            assert all(np.isnan(t[0]) for t in LR.point(q, [mu_], [var_])), (kind, mu_, var_)
            assert np.all(np.isnan(program(kind, s, 0.5, 0.0, [mu_], [var_]))), (kind, mu_, var_)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_minus_infinity_only_below_the_doubles(kind, program):
    """finite moments with var > 0: log alpha is finite as far as z^2 / 2 is a double, and -inf beyond"""
    z = np.array([-1e150, -1.8e154, -1.89e154, -2e154, -1e200])  # z^2 / 2 = 5e299, 1.62e308, 1.786e308, 2e308 (> DBL_MAX), 5e399
    for got in (LR.point(LR.acq(kind), z, np.ones_like(z))[0], program(kind, 1.0, 0.0, 0.0, z, np.ones_like(z))[0]):
        assert np.all(np.isfinite(got[:3])) and np.all(np.isneginf(got[3:])), got
        half = (z[:3] / 2) * z[:3]
        assert np.all(np.abs(got[:3] + half) <= 4 * EPS * half)


# ---- against the plain kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("minimize", [False, True])
def test_exp_of_the_log_kinds_is_the_plain_kinds(kind, minimize):
    """exp(LogEI) = EI, exp(LogPI) = PI and d log alpha = d alpha / alpha within PARITY wherever the plain value is a normal number: the
    901 points of z in [-37, 8] of tests/test_acq_host.py at three sigmas, and the grid of this file"""
    s = -1.0 if minimize else 1.0
    mu0, var0 = plain_grid_moments()
    mu1, var1 = LR.grid_moments(s)
    mu, var = np.concatenate([s * mu0, mu1]), np.concatenate([var0, var1])
    pa, pm, ps, _ = A.point(A.acq(LR.PLAIN[kind], minimize=minimize), mu, var)
    la, lm, ls, _ = LR.point(LR.acq(kind, minimize=minimize), mu, var)
    normal = pa >= np.finfo(np.float64).tiny
    assert normal.sum() > 2700 and (~normal).sum() >= 15  # (the far tail is where the plain kinds have nothing to compare with)
    with np.errstate(all="ignore"):
        e = [np.max(LR.err_rel(np.exp(la[normal]), pa[normal])), np.max(LR.err_rel(lm[normal] * pa[normal], pm[normal])),
             np.max(LR.err_rel(ls[normal] * pa[normal], ps[normal]))]
    print(f"{kind} s={s:+.0f}: exp(log alpha) against alpha {e[0]:.2e}, the derivatives times alpha {e[1]:.2e} {e[2]:.2e}")
    assert max(e) <= PARITY


# ---- the plateau case of the GPU suite --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain,kind", LR.PLATEAU_KINDS)
def test_plateau_case_on_the_oracle(plain, kind):
    """on the oracle's objects: the plain kind and its gradient are exactly 0 at every start; the log kind's trajectory is conditioned
    (float64 against long double within _acq_ref.COND_CAP), every start climbs, and the two best values are further apart than GAP"""
    parts = LR.plateau_oracle_parts()
    X0, lo, hi, lr = LR.plateau_inputs()
    T = LR.PLATEAU["T"]
    best = LR.plateau_best(parts, X0, lo, hi)
    x0 = np.minimum(np.maximum(X0, lo), hi)
    assert X0[0, 0] > hi[0] and len(X0) == 8 and T == 30
    pa, pg, mu, var = A.alpha_grad(A.acq(plain, best=best), x0, parts)
    assert np.all((mu - best) / np.sqrt(var) <= -LR.PLATEAU["sds"])
    assert np.all(pa == 0.0) and np.all(pg == 0.0)
    px, pA = A.ascent(A.acq(plain, best=best), X0, parts, lo, hi, lr, T)
    assert np.array_equal(px, x0) and np.all(pA == 0.0)
    q = LR.acq(kind, best=best)
    x64, a64 = LR.ascent(q, X0, parts, lo, hi, lr, T)
    xl, al = LR.ascent(q, X0, parts, lo, hi, lr, T, dtype=np.longdouble)
    cx, ca, gap = float(np.max(np.abs(x64 - xl)) / np.max(hi - lo)), A.relerr(a64, al), A.top_gap(a64)
    print(f"{kind}: conditioning x {cx:.1e} of the box, log alpha {ca:.1e}, top gap {gap:.1e}")
    assert cx <= A.COND_CAP and ca <= A.COND_CAP and gap > A.GAP
    a0 = LR.alpha_grad(q, x0, parts)[0]
    assert np.all(np.isfinite(a0)) and np.all(a64 > a0) and not np.any(x64 == x0)


# ---- the host mirror ----------------------------------------------------------------------------------------------------------------------------
def test_mirror_classes_and_constants():
    import agp_amd as AGP
    from agp_amd import capi
    from agp_amd.acquisition import _Acquisition

    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agp_hip.h")).read(), flags=re.S)
    enum = dict((k, int(v)) for k, v in re.findall(r"(AGP_ACQ_[A-Z_]+)\s*=\s*(\d+)", h))
    assert enum == {"AGP_ACQ_UCB": 0, "AGP_ACQ_EI": 1, "AGP_ACQ_PI": 2, "AGP_ACQ_LOG": 4, "AGP_ACQ_LOG_EI": 5, "AGP_ACQ_LOG_PI": 6}
    assert (capi.ACQ_LOG, capi.ACQ_LOG_EI, capi.ACQ_LOG_PI) == (enum["AGP_ACQ_LOG"], enum["AGP_ACQ_LOG_EI"], enum["AGP_ACQ_LOG_PI"]) == (4, 5, 6)
    assert capi.ACQ_LOG_EI == capi.ACQ_LOG | capi.ACQ_EI and capi.ACQ_LOG_PI == capi.ACQ_LOG | capi.ACQ_PI
    assert LR.CODES == {"logei": capi.ACQ_LOG_EI, "logpi": capi.ACQ_LOG_PI}
    for cls, code, name in ((AGP.LogEI, 5, "LogEI"), (AGP.LogPI, 6, "LogPI")):
        a = cls(best=0.25, xi=0.5)
        assert isinstance(a, _Acquisition) and a.kind == code and repr(a) == f"{name}(best=0.25, xi=0.5)"
        assert repr(cls()) == f"{name}(best=None, xi=0.0)" and cls().best is None
        d = a.desc(True)
        assert (d.kind, d.minimize, d.beta, d.best, d.xi) == (code, 1, 0.0, 0.25, 0.5)
        assert cls().desc(False, best=1.5).best == 1.5
        for bad in (lambda: cls(0.0, xi=-0.1), lambda: cls(0.0, xi=float("inf")), lambda: cls(float("nan")), lambda: cls(float("inf"))):
            with pytest.raises(ValueError):
                bad()
    # the plain kinds are what they were
    assert (AGP.UCB().kind, AGP.EI().kind, AGP.PI().kind) == (0, 1, 2) and repr(AGP.EI(0.5)) == "EI(best=0.5, xi=0.0)"


def test_mirror_argument_checks():
    import agp_amd as AGP

    Z = np.random.default_rng(0).standard_normal((5, 3))
    model = AGP.SVGP(AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), Z, optimiser=False)
    X = np.zeros((4, 3))
    for call in (lambda a: AGP.acquisition(model, a, X), lambda a: AGP.maximize_acquisition(model, a, X, (-1.0, 1.0)),
                 lambda a: AGP.maximize_acquisition_batch(model, a, 2, X, (-1.0, 1.0)), lambda a: AGP.acquisition_moments(a, np.zeros(3), np.ones(3))):
        for bad in ("logei", 5, AGP.LogEI, None):  # (the class is not an instance)
            with pytest.raises(TypeError, match="LogEI"):
                call(bad)
    for cls in (AGP.LogEI, AGP.LogPI):
        with pytest.raises(ValueError, match="best must be given"):
            AGP.acquisition_moments(cls(), np.zeros(3), np.ones(3))
        for call in (lambda a: AGP.acquisition(model, a, X), lambda a: AGP.maximize_acquisition(model, a, X, (-1.0, 1.0)),
                     lambda a: AGP.maximize_acquisition_batch(model, a, 2, X, (-1.0, 1.0)),
                     lambda a: AGP.acquisition(model, a, X, pending=X[:2])):
            with pytest.raises(ValueError, match="best=None"):  # an SVGP has no training inputs to take the incumbent from
                call(cls())
        a = cls(0.0)
        a.xi = -1.0  # (changed after construction: checked again at the call)
        with pytest.raises(ValueError, match="xi"):
            AGP.acquisition(model, a, X)
        f32 = AGP.SVGP(AGP.SqExponentialKernel(), AGP.GaussianLikelihood(0.1), AGP.AnalyticVI(), Z, optimiser=False, T=np.float32)
        with pytest.raises(NotImplementedError, match="Float32"):  # the refusals are those of the plain kinds
            AGP.acquisition(f32, cls(0.0), X)
