"""The per-round scratch of the tile factorisation (chol_rounds in csrc/agp_chol.h: four raw panel columns P and four M rows Mw)
is laid out in 16-byte groups so that every LDS read of a round is a full-rate one.  The layout is private to the rounds; a slip
between its publish and its read side shows up in two places that the rest of the suite does not pin:

* the M rows.  Only the tile factorisation's own residual check (agp_dev_diag_bench: ||L L' - A||, ||X L - I|| and the strict-upper
  leakage of one 64 x 64 tile, tolerances 1e-12 / 1e-4) sees the inverse that the M rows build; the potrf residual tests look at L
  alone.  Variants 1 (2-level, full inverse) and 13 (2-level without X21) in fp64, 1 in fp32: every call must return 0.  These are
  the variants the library has; any other (the rejected 1-level, minors and panel forms and their timing experiments, removed) must
  return AGP_ERR_INVALID, without a launch.
* the bits.  A layout change moves values, it does no arithmetic: factors, variational parameters and the ELBO must equal, bit for
  bit, those of the build before the layout changed.  tests/golden/round_layout_hashes.json holds their SHA-256 hashes (ELBO:
  float.hex), produced by tools/round_layout_golden.py ON THE PARENT COMMIT'S BUILD on an MI355X: agp_potrf_jitter factors at
  n = 64, 96, 200 in both types, and mu, Sigma, ELBO of an SVGP after 5 CAVI steps at m = 128, 192 (2 and 3 block columns) with
  batches of 64 and 200 (ragged), where get_state takes the pending step through flush().  The file is regenerated only by a change
  that alters arithmetic on purpose.  Under a fallback-forcing variable (tests/_knobs.py) other kernels with another summation order
  run, so the hash assertions are skipped there."""
import ctypes as C
import importlib.util
import json
import os

import pytest

import _knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGP_ERR_INVALID = 1  # include/agp_hip.h, agp_status


def _golden_tool():
    spec = importlib.util.spec_from_file_location("round_layout_golden", os.path.join(ROOT, "tools", "round_layout_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool(built):
    import torch

    assert torch.cuda.is_available()
    return _golden_tool()


@pytest.fixture(scope="module")
def golden(tool):
    with open(tool.GOLDEN) as fh:
        return json.load(fh)


def _skip_if_forced():
    if _knobs.forced(*_knobs._DEFAULTS):
        pytest.skip("a fallback-forcing variable is set: other kernels, other summation order")


def _diag_bench(cases):
    """[(dt, variant, status of agp_dev_diag_bench(ctx, dt, variant, 1, 2, &us))] on one context"""
    import torch
    from agp_amd import capi

    L = capi.lib()
    f = L.agp_dev_diag_bench
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        us = C.c_double()
        return [(dt, variant, f(ctx, dt, variant, 1, 2, C.byref(us))) for dt, variant in cases]
    finally:
        L.agp_ctx_destroy(ctx)


@pytest.mark.parametrize("dt,variant", [(0, 1), (0, 13), (1, 1)])
def test_tile_factorisation_residuals_with_the_inverse(built, dt, variant):
    assert _diag_bench([(dt, variant)]) == [(dt, variant, 0)]


def test_removed_tile_factorisation_variants_are_invalid(built):
    cases = [(0, 0), (0, 2), (0, 8), (1, 13)]
    assert _diag_bench(cases) == [(dt, variant, AGP_ERR_INVALID) for dt, variant in cases]


@pytest.mark.parametrize("dn", ["f64", "f32"])
@pytest.mark.parametrize("n", [64, 96, 200])
def test_potrf_factor_bits_equal_the_parent_build(tool, golden, n, dn):
    _skip_if_forced()
    assert tool.potrf_hash(n, 0 if dn == "f64" else 1) == golden[f"potrf_{dn}_n{n}"]


@pytest.mark.parametrize("m,B", [(128, 64), (128, 200), (192, 64), (192, 200)])
def test_svgp_state_and_elbo_bits_equal_the_parent_build(tool, golden, m, B):
    _skip_if_forced()
    got = tool.svgp_hashes(m, B)
    print(got)
    assert got == golden[f"svgp_m{m}_B{B}"]
