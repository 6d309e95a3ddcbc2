"""CPU tests of the input gradients of pathwise samples: the restatement tests/_pathwise_grad_ref.py against central differences of
the restated paths (tests/_pathwise_ref.py), and what the host mirror decides without a device -- the binding, the freed draw, the
refusal of the ExponentialKernel in the words the header documents."""
import os

import numpy as np
import pytest

import _pathwise_grad_ref as PG
import _pathwise_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2 = 1.5
CASES = {"D1": (1, 2.0), "D3-ard": (3, (0.7, 1.9, 3.1)), "D5": (5, 1.3)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", ["sqexponential", "matern52", "matern32"])
def test_restatement_against_central_differences(kind, case):
    """m = 65, S = 7, 130 features, 40 standard-normal points of which the first five lie exactly on inducing points, V a random
    table; central differences of Draw.__call__ with h = 1e-6 (at 1e-5 the third-derivative term of Matern-3/2 shows)."""
    D, scale = CASES[case]
    rng = np.random.default_rng(100 + D)
    m, S, nf, nt, h = 65, 7, 130, 40, 1e-6
    Z = rng.standard_normal((m, D))
    d = P.Draw(kind, scale, SIGMA2, Z, S, nf, seed=4711, t=D)
    d.V = rng.standard_normal((m, S))
    X = rng.standard_normal((nt, D))
    X[:5] = Z[:5]
    G = PG.grad(d, X)
    assert G.shape == (S, nt, D) and np.all(np.isfinite(G))
    FD = np.empty_like(G)
    for k in range(D):
        e = np.zeros(D)
        e[k] = h
        FD[:, :, k] = (d(X + e) - d(X - e)) / (2 * h)
    err = float(np.max(np.abs(FD - G)) / np.max(np.abs(G)))
    print(f"{kind}, {case}: max|FD - G| / max|G| = {err:.2e}")
    assert err < 1e-8


def test_restatement_refuses_the_exponential_kernel():
    with pytest.raises(NotImplementedError, match="ExponentialKernel"):
        PG.dphi("exponential", np.ones(3))


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
def test_binding_and_exported_symbol(built):
    import agp_amd as AGP
    from agp_amd import capi

    assert callable(AGP.PathwiseSamples.grad)
    res, args = capi.SYMBOLS["agp_pathwise_eval_grad"]
    assert len(args) == 9
    assert capi.lib().agp_pathwise_eval_grad.argtypes == args  # the library exports it


def _hollow(kinds, freed):
    """a PathwiseSamples with no device object behind it: what grad decides on the host is decided before it needs one"""
    from agp_amd.pathwise import PathwiseSamples

    ps = PathwiseSamples.__new__(PathwiseSamples)
    ps._model, ps._kinds, ps._p = None, tuple(kinds), None if freed else object()
    ps.n_latent, ps.n_samples, ps.D = len(kinds), 2, 3
    return ps


def test_grad_on_a_freed_draw_raises():
    from agp_amd import capi

    with pytest.raises(RuntimeError, match="freed"):
        _hollow([capi.K_SQEXP], freed=True).grad(np.zeros((4, 3)))


def test_exponential_refusal_is_the_documented_string():
    from agp_amd import capi, pathwise

    text = pathwise.GRAD_REFUSAL_EXPONENTIAL
    assert text == "ExponentialKernel is not differentiable at zero distance"
    with open(os.path.join(ROOT, "include", "agp_hip.h")) as f:
        header = f.read()
    doc = header[header.index(" * agp_pathwise_eval_grad "):header.index(" * agp_pathwise_get ")]
    assert text in doc and "AGP_ERR_UNSUPPORTED" in doc
    for kinds in ([capi.K_EXPONENTIAL], [capi.K_MATERN52, capi.K_EXPONENTIAL]):  # any latent of the draw
        with pytest.raises(NotImplementedError) as ei:
            _hollow(kinds, freed=False).grad(np.zeros((4, 3)))  # (no model, no device: refused before either is touched)
        assert text in str(ei.value)
