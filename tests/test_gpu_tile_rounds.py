"""The 4-column rounds of the diagonal-tile factorisation (chol_rounds in csrc/agp_chol.h) issue all their LDS reads in front of the
pivot block's LDL' and store the four raw pivots at the end of the round.  Two things the rest of the suite does not pin:

* the index of a failed pivot at every position inside a round (column 0 .. 3 of its 4x4 pivot block), at the first and last round
  of a 16-column group, on both sides of the 32-column boundary between the two eliminations of a tile and of the 64-column
  boundary between tiles, and in the first, a middle and the last block column of the matrix;
* the factor itself where tiles are full, partly valid and several: ||L L' - A|| / ||A|| (max norm) <= 4 n u, the n u shape of the
  backward error of Cholesky (u = 2^-53 / 2^-24) -- numpy.linalg.cholesky leaves 0.016 - 0.027 n u on these matrices, so a correct
  factor has two orders of magnitude of room and a wrong one none.

Every case factors one matrix through agp_potrf_jitter (jitter 0) on a context of its own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SPD = {}


def _spd(n):
    """A = G G' / n + I / 2 with G n x (n + 8), seeded by n; computed once per n and never modified (callers copy)"""
    if n not in _SPD:
        G = np.random.default_rng(n).standard_normal((n, n + 8))
        A = G @ G.T / n + 0.5 * np.eye(n)
        A.setflags(write=False)
        _SPD[n] = A
    return _SPD[n]


@pytest.fixture(scope="module")
def mods(built):
    import torch

    assert torch.cuda.is_available()
    from agp_amd import capi

    return capi, torch


def _potrf(mods, A, dt):
    """factor a copy of A (numpy, fp64) in the library's type dt (0: fp64, 1: fp32) -> (status, info, what was factored, result)"""
    capi, torch = mods
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.agp_ctx_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ctx)) == 0
    try:
        n = A.shape[0]
        ad = torch.tensor(A, dtype=torch.float32 if dt else torch.float64, device="cuda").contiguous()
        given = ad.cpu().numpy().astype(np.float64)
        info = C.c_int32(-7)
        st = L.agp_potrf_jitter(ctx, dt, C.c_void_p(ad.data_ptr()), n, n, 0.0, C.byref(info))
        torch.cuda.synchronize()
        return st, info.value, given, ad.cpu().numpy().astype(np.float64)
    finally:
        L.agp_ctx_destroy(ctx)


BAD64 = [0, 1, 2, 3, 4, 15, 16, 31, 32, 35, 63, 64, 67, 127, 128, 191]
BAD32 = [0, 3, 32, 64, 191]


@pytest.mark.parametrize("dt,bad", [(0, b) for b in BAD64] + [(1, b) for b in BAD32])
def test_failed_pivot_index_inside_rounds_and_at_block_boundaries(mods, dt, bad):
    """n = 192 (three block columns).  The leading bad x bad block is a principal block of an SPD matrix and the Schur complement at
    `bad` is at most A[bad, bad] = -1, so the first non-positive leading minor is bad + 1 exactly (status 2 = AGP_ERR_NOT_POSDEF)."""
    A = _spd(192).copy()
    A[bad, bad] = -1.0
    st, info, _, _ = _potrf(mods, A, dt)
    assert st == 2 and info == bad + 1, (st, info)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("n", [64, 96, 128, 200])  # one tile, a partly valid last tile, two tiles, three tiles + a partial one
def test_factor_residual_at_tile_edges(mods, n, dt):
    st, info, given, out = _potrf(mods, _spd(n), dt)
    assert st == 0 and info == 0, (st, info)
    Lf = np.tril(out)
    res = np.abs(Lf @ Lf.T - given).max() / np.abs(given).max()
    bound = 4 * n * (2.0 ** -24 if dt else 2.0 ** -53)
    print(f"n = {n} {'f32' if dt else 'f64'}: residual {res:.3e}, bound {bound:.3e}")
    assert res <= bound, (res, bound)
