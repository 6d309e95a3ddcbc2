"""The Cholesky building blocks (agp_potrf_jitter, agp_spd_inverse, agp_solve_right_spd) on ill-conditioned, badly scaled, singular and
NaN-carrying matrices.  Families, reference, metrics, the plain model and the budget are defined in tests/_chol_ref.py (and checked
on the host by tests/test_chol_budget_host.py); the library is always called with jitter 0 on a matrix already rounded to its type.

Accuracy: every case of _chol_ref.accuracy_cases (n = 136: three block columns, 8 valid columns in the last; n = 328: six), both
types, on the default driver (the task graph at these sizes) and once more under AGP_CHOL_DAG=0 (k_chol_step, trtri_levels) in one
child process whose results the parent holds to the same budgets.  n = 6144 reaches the blocked driver: the factor only, by
eta_sampled against 4 eta_sampled(LAPACK in T).

Failure reporting: an exactly zero pivot (singular(n, r)) and a NaN in the input must come back as status 2 (AGP_ERR_NOT_POSDEF) with
info = first_bad_pivot(A), from agp_potrf_jitter and from agp_spd_inverse, both types, both small-size drivers; the same context then
factors a good matrix correctly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _chol_ref as R
import _knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f64", "f32")
CASES = [(f, n, p, dt) for dt in DTYPES for (f, n, p) in R.accuracy_cases(dt)]
IDS = [R.case_id(*c) for c in CASES]
FAILURES = [("singular", n, r) for (n, r) in R.SINGULAR] + [("nan", i, k) for (i, k) in R.NAN_AT]
FAIL_IDS = [f"{k}-{a}-{b}" for (k, a, b) in FAILURES]
DRIVERS = ("default", "nodag")


def _bad_matrix(kind, a, b):
    return R.singular(a, b) if kind == "singular" else R.with_nan(R.NAN_N, a, b)


# ---- the device side: used in this process (default driver) and in the child (AGP_CHOL_DAG=0) ------------------------------------------
class _Dev:
    def __init__(self):
        import torch
        from agp_amd import capi

        assert torch.cuda.is_available()
        self.torch, self.L = torch, capi.lib()

    def ctx(self):
        ctx = C.c_void_p()
        assert self.L.agp_ctx_create(0, C.c_void_p(self.torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
        return ctx

    def put(self, A, dtype):
        return self.torch.tensor(A, dtype=self.torch.float32 if dtype == "f32" else self.torch.float64, device="cuda").contiguous()

    def potrf(self, ctx, A, dtype):
        """-> (status, info, the n x n array the call leaves)"""
        n = A.shape[0]
        ad = self.put(A, dtype)
        info = C.c_int32(-7)
        st = self.L.agp_potrf_jitter(ctx, R.DT[dtype], C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        self.torch.cuda.synchronize()
        return st, info.value, ad.cpu().numpy().astype(np.float64)

    def inverse(self, ctx, A, dtype):
        """-> (status, info, A^-1, logdet)"""
        n = A.shape[0]
        ad = self.put(A, dtype)
        inv = self.torch.zeros_like(ad)
        info, ld = C.c_int32(-7), C.c_double(np.nan)
        st = self.L.agp_spd_inverse(ctx, R.DT[dtype], C.c_void_p(ad.data_ptr()), n, n, C.c_void_p(inv.data_ptr()), n, C.byref(ld),
                                    C.byref(info))
        self.torch.cuda.synchronize()
        return st, info.value, inv.cpu().numpy().astype(np.float64), ld.value

    def solve(self, ctx, A, B, dtype):
        """-> (status, info, X = B A^-1)"""
        n, r = A.shape[0], B.shape[0]
        ad, bd = self.put(A, dtype), self.put(B, dtype)
        xd = self.torch.zeros_like(bd)
        info = C.c_int32(-7)
        st = self.L.agp_solve_right_spd(ctx, R.DT[dtype], C.c_void_p(ad.data_ptr()), n, n, C.c_void_p(bd.data_ptr()), n, r,
                                        C.c_void_p(xd.data_ptr()), n, C.byref(info))
        self.torch.cuda.synchronize()
        return st, info.value, xd.cpu().numpy().astype(np.float64)

    def accuracy(self, A, B, dtype):
        """the three building blocks on one matrix, on a context of its own"""
        ctx = self.ctx()
        try:
            st, info, out = self.potrf(ctx, A, dtype)
            sti, infoi, Y, ld = self.inverse(ctx, A, dtype)
            sts, infos, Xs = self.solve(ctx, A, B, dtype)
        finally:
            self.L.agp_ctx_destroy(ctx)
        return {"status": np.array([st, info, sti, infoi, sts, infos]), "L": out, "Y": Y, "logdet": np.array(ld), "X": Xs}

    def failure(self, bad, good, dtype):
        """[status, info] of agp_potrf_jitter and of agp_spd_inverse on `bad`, then of agp_potrf_jitter on `good` in the same context,
        and that factor"""
        ctx = self.ctx()
        try:
            st, info, _ = self.potrf(ctx, bad, dtype)
            sti, infoi, _, _ = self.inverse(ctx, bad, dtype)
            stg, infog, Lg = self.potrf(ctx, good, dtype)
        finally:
            self.L.agp_ctx_destroy(ctx)
        return {"status": np.array([st, info, sti, infoi, stg, infog]), "L": Lg}


def _fail_key(kind, a, b, dtype):
    return f"fail-{kind}-{a}-{b}-{dtype}"


def _run_accuracy(dev, case):
    f, n, p, dt = case
    return dev.accuracy(R.FAMILY[f](n, p, dt), R.rhs(n, dt), dt)


def _run_failure(dev, fail, dtype):
    bad = _bad_matrix(*fail)
    return dev.failure(bad, R.spd0(bad.shape[0]), dtype)


def _child(path):
    """every small case on this process's driver -> one .npz"""
    dev, out = _Dev(), {}
    for case in CASES:
        for k, v in _run_accuracy(dev, case).items():
            out[f"{R.case_id(*case)}|{k}"] = v
    for fail in FAILURES:
        for dt in DTYPES:
            for k, v in _run_failure(dev, fail, dt).items():
                out[f"{_fail_key(*fail, dt)}|{k}"] = v
    np.savez(path, **out)


_CHILD = ("import sys; sys.path[:0] = ['.', 'tests']; import __graft_entry__ as g; g.build(); "
          "import test_gpu_chol_conditioning as M; M._child(sys.argv[1])")
_state = {}


@pytest.fixture(scope="module")
def dev(built):
    return _Dev()


@pytest.fixture(scope="module")
def nodag(built, tmp_path_factory):
    """the child process under AGP_CHOL_DAG=0, run once: key -> {name: array}"""
    path = str(tmp_path_factory.mktemp("chol_nodag") / "results.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=ROOT, env=dict(os.environ, AGP_CHOL_DAG="0"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    with np.load(path) as z:
        for key in z.files:
            k, name = key.split("|")
            out.setdefault(k, {})[name] = z[key]
    return out


def _results(request, driver, key, run):
    """what the device returned for `key` on `driver`: computed once and shared by the tests that look at it"""
    if driver == "nodag":
        if _knobs.no_task_graph():
            pytest.skip("AGP_CHOL_DAG=0 is this run's setting already: the default-driver cases cover it")
        return request.getfixturevalue("nodag")[key]
    if key not in _state:
        _state[key] = run(request.getfixturevalue("dev"))
    return _state[key]


def _line(c, driver, got, names):
    u = c.u
    print(f"{c.id} [{driver}] " + "  ".join(
        f"{m}: kernel {got[m] / u:.4g} u, model {c.model[m] / u:.4g} u, LAPACK {c.lapack[m] / u:.4g} u" for m in names))


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_potrf_within_budget(request, case, driver):
    c = R.case(*case)
    res = _results(request, driver, c.id, lambda d: _run_accuracy(d, case))
    st, info = res["status"][:2]
    assert st == 0 and info == 0, (st, info)
    out = res["L"]
    assert np.all(np.isfinite(out))
    assert not np.triu(out, 1).any(), "the strict upper triangle is zero"
    got = R.measure(c, L=out)
    _line(c, driver, got, ("eta", "phi"))
    assert got["eta"] <= c.budget["eta"], (got["eta"] / c.u, c.budget["eta"] / c.u)
    assert got["phi"] <= c.budget["phi"], (got["phi"] / c.u, c.budget["phi"] / c.u)


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spd_inverse_within_budget(request, case, driver):
    c = R.case(*case)
    res = _results(request, driver, c.id, lambda d: _run_accuracy(d, case))
    st, info = res["status"][2:4]
    assert st == 0 and info == 0, (st, info)
    Y, ld = res["Y"], float(res["logdet"])
    assert np.all(np.isfinite(Y))
    got = R.measure(c, Y=Y)
    err = abs(float(R.LD(ld) - c.logdet_ref))
    _line(c, driver, got, ("psi",))
    print(f"{c.id} [{driver}] logdet: kernel off by {err:.3e}, model by {abs(c.model_logdet - float(c.logdet_ref)):.3e}, "
          f"bound {c.budget['logdet']:.3e}")
    assert got["psi"] <= c.budget["psi"], (got["psi"] / c.u, c.budget["psi"] / c.u)
    assert err <= c.budget["logdet"], (err, c.budget["logdet"])
    assert np.array_equal(Y, Y.T), "A^-1 = X' X is symmetric to the bit"


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_solve_right_within_budget(request, case, driver):
    c = R.case(*case)
    res = _results(request, driver, c.id, lambda d: _run_accuracy(d, case))
    st, info = res["status"][4:6]
    assert st == 0 and info == 0, (st, info)
    assert np.all(np.isfinite(res["X"]))
    got = R.measure(c, Xs=res["X"])
    _line(c, driver, got, ("chi",))
    assert got["chi"] <= c.budget["chi"], (got["chi"] / c.u, c.budget["chi"] / c.u)


@pytest.mark.parametrize("dtype", DTYPES)
def test_blocked_potrf_within_budget(dev, dtype):
    """n = 6144, 96 block rows: the blocked driver (diagonal block / panel / trailing launches)"""
    c = R.big_case(dtype)
    ctx = dev.ctx()
    try:
        st, info, out = dev.potrf(ctx, c.A, dtype)
    finally:
        dev.L.agp_ctx_destroy(ctx)
    assert st == 0 and info == 0, (st, info)
    assert not np.triu(out, 1).any()
    got = R.eta_sampled(c.A, out)
    print(f"{c.id} [blocked] eta_sampled: kernel {got / c.u:.4g} u, LAPACK {c.lapack['eta'] / c.u:.4g} u")
    assert got <= c.budget["eta"], (got / c.u, c.budget["eta"] / c.u)


# ---- failure reporting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fail", FAILURES, ids=FAIL_IDS)
def test_zero_and_nan_pivots_are_reported_at_their_index(request, fail, dtype, driver):
    bad = _bad_matrix(*fail)
    n = bad.shape[0]
    want = R.first_bad_pivot(bad)
    assert want == (fail[2] if fail[0] == "singular" else fail[1]) + 1
    res = _results(request, driver, _fail_key(*fail, dtype), lambda d: _run_failure(d, fail, dtype))
    st, info, sti, infoi, stg, infog = (int(v) for v in res["status"])
    print(f"{fail} {dtype} [{driver}]: potrf ({st}, {info}), spd_inverse ({sti}, {infoi}), expected (2, {want})")
    assert (st, info) == (2, want), ("agp_potrf_jitter", st, info, want)
    assert (sti, infoi) == (2, want), ("agp_spd_inverse", sti, infoi, want)
    # the same context afterwards: the suite's well-conditioned matrix, to the suite's 4 n u (tests/test_gpu_tile_rounds.py)
    assert (stg, infog) == (0, 0), (stg, infog)
    good = R.spd0(n).astype(R.NPT[dtype]).astype(np.float64)
    Lg = res["L"]
    assert not np.triu(Lg, 1).any()
    assert np.abs(Lg @ Lg.T - good).max() / np.abs(good).max() <= 4 * n * R.U[dtype]
