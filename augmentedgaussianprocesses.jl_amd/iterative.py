"""IterativeGP -- the exact GP without an N x N matrix, and the two operators it runs on: `kernel_matmul`, (K(X, Y) + c I) V for a block
V with K never in memory (agp_kernel_matmul, csrc/agp_kmv.h), and `kernel_bilinear_grad`, sum_c w_c u_c' (dK / d theta) v_c for the
kernel's variance and scales with neither K nor the weight matrix in memory (agp_kernel_bilinear_grad, csrc/agp_kmv_grad.h), under a
batched preconditioned CG (agp_gp_cg_*).  N is limited by time, not by 8 N^2 bytes.  Float64, D <= 128, one GPU, Gaussian likelihood;
the operator product alone also has a Float32 instance (csrc/agp_kmv_f32.h: `kernel_matmul(dtype=np.float32)`,
`IterativeGP(operator_dtype=np.float32)`).  `block=128` on either takes 128 columns per launch / per CG run (csrc/agp_kmv_wide.h).
65 <= D <= 128 runs on a kernel of its own (agp_kernel_matmul_hd, csrc/agp_kmv_hd.h): the Float64 product of up to 32 columns, and
with it solve, operator, alpha, predict_f, predict_y and the log marginal likelihood without gradients.  The Float32 operator, the
block of 128 and every derivative or path kernel stop at D = 64 and say so.

The log marginal likelihood is stochastic: log det(K + noise I) = log det P + E_z[z' P^-1/2 log(P^-1/2 (K + noise I) P^-1/2) P^-1/2 z]
over probes z ~ N(0, P), P the solver's preconditioner, each expectation term by Lanczos quadrature on the coefficients the CG
computes anyway; the trace in the gradient uses the same probes and solves.  `IterativeGP.optimize` takes ascent steps on it.
`train_` stays refused (it is the interface of the variational models).  `kernel_matmul_grad` is the derivative of the operator
product with respect to its row points (agp_kernel_matmul_dx, csrc/agp_kmv_dx.h); `predict_f_grad(IterativeGP)` runs on it.
`sample_paths(IterativeGP, S)` draws posterior functions without an N x N matrix (pathwise.py: IterativePaths; the fused
path-evaluation kernel of csrc/agp_path.h under the draw's batched CG and under every evaluation; paths(X, dtype=np.float32) evaluates on its Float32 instance, csrc/agp_path_f32.h).  Not here: the full predictive
covariance, gradients with respect to the training inputs or the prior mean, gradients of the drawn paths.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from .likelihoods import GaussianLikelihood
from .svgp import ADAM, ELBO, predict_f, predict_y, train_

MAXR = 32  # right-hand sides per launch / per batched solve (KMV_MAXR)
MAXD = 64  # input dimensions of every operator kernel but the Float64 product of 32 columns (KMV_MAXD), whose limit is
HD_MAXD = 128  # (KMV_HD_MAXD: agp_kernel_matmul_hd, csrc/agp_kmv_hd.h)
WIDE = 128  # ... of the wide block (KMV_WIDE_MAXR): kernel_matmul(block=128), IterativeGP(block=128)


def _block(block, who):
    if isinstance(block, bool) or block not in (MAXR, WIDE):
        raise ValueError(f"{who}: block must be 32 or 128, got {block!r}")
    return int(block)


def _refuse_hd(D, who, what, exc=NotImplementedError):
    """what has no kernel for 65 .. 128 input dimensions is refused by name"""
    if D > MAXD:
        raise exc(f"{who}: D = {D}, but {what} stops at D = {MAXD} (only the Float64 operator product of 32 columns serves "
                  f"{MAXD + 1} <= D <= {HD_MAXD})")


def _torch():
    import torch

    return torch


class _Ctx:
    """a context of the C ABI on the current device and stream"""

    def __init__(self, device: Optional[int] = None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: augmentedgaussianprocesses.jl_amd has no CPU fallback")
        self.dev = torch.device("cuda", device if device is not None else torch.cuda.current_device())
        self.ctx = C.c_void_p()
        self.refs = 1  # the owner; a paths object drawn on this context holds another (retain) and outlives the model's close()
        st = capi.lib().agp_ctx_create(self.dev.index, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream), C.byref(self.ctx))
        if st != capi.AGP_OK:
            raise capi.AGPError(st, "agp_ctx_create failed")

    def chk(self, st):
        capi.check(self.ctx, st)

    def dev_tensor(self, A, dtype=np.float64):
        torch = _torch()
        t = A.to(device=self.dev, dtype=_torch_dtype(dtype)) if isinstance(A, torch.Tensor) else torch.as_tensor(
            np.array(A, dtype=dtype), device=self.dev)
        return t[:, None] if t.ndim == 1 else t

    def retain(self):
        self.refs += 1
        return self

    def close(self):
        self.refs -= 1
        if self.ctx and self.refs <= 0:
            capi.lib().agp_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()


def _np_dtype(dtype, what):
    """np.float64 or np.float32 as a NumPy scalar type; anything else is refused by name"""
    try:
        dt = np.dtype(dtype).type
    except TypeError:
        dt = None
    if dt not in (np.float64, np.float32):
        raise ValueError(f"{what} must be np.float64 or np.float32, got {dtype!r}")
    return dt


def _torch_dtype(dtype):
    return _torch().float32 if dtype is np.float32 else _torch().float64


def _rows(t):
    """a 2-D device tensor whose rows are contiguous (any row pitch is fine for the ABI)"""
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _kernel_matmul(cx, kernel, Xd, Vd, Yd, diag_add, col_groups, dtype=np.float64, block=MAXR):
    torch = _torch()
    L = capi.lib()
    sym = Yd is None
    Xd, Vd = _rows(Xd), _rows(Vd)
    Yd = None if sym else _rows(Yd)
    n, D = Xd.shape
    p = n if sym else Yd.shape[0]
    if Vd.shape[0] != p:
        raise ValueError(f"V has {Vd.shape[0]} rows, K(X, Y) has {p} columns")
    kd, keep = kernel.desc(D)
    out = torch.empty(n, Vd.shape[1], dtype=_torch_dtype(dtype), device=cx.dev)
    call = L.agp_kernel_matmul_hd if D > MAXD else L.agp_kernel_matmul_wide if block == WIDE else L.agp_kernel_matmul
    for c0 in range(0, Vd.shape[1], block):
        v, o = Vd[:, c0:c0 + block], out[:, c0:c0 + block]
        cx.chk(call(cx.ctx, capi.F32 if dtype is np.float32 else capi.F64, C.byref(kd), C.c_void_p(Xd.data_ptr()), n, Xd.stride(0),
                    None if sym else C.c_void_p(Yd.data_ptr()), p, 0 if sym else Yd.stride(0), D, 1 if sym else 0,
                    float(diag_add), C.c_void_p(v.data_ptr()), Vd.stride(0), v.shape[1], int(col_groups),
                    C.c_void_p(o.data_ptr()), out.stride(0)))
    del keep
    return out


def kernel_matmul(kernel, X, V, Y=None, diag_add: float = 0.0, col_groups: int = 0, device: Optional[int] = None, dtype=np.float64,
                  block: int = 32):
    """(K(X, Y) + diag_add I) V on the device without forming K.  X: n x D, Y: p x D, V: p x r (a vector counts as p x 1); Y=None is
    the symmetric form K(X, X) + diag_add I, with an exact diagonal.  diag_add needs Y=None.  More than `block` columns are taken in
    blocks of `block` (32, or 128: see below).  col_groups: 0 lets the library split the columns of K over workgroups; a positive value forces that many groups.
    Arrays in, a NumPy array out; device tensors in, a device tensor out.  dtype: np.float64 (default) or np.float32 -- the inputs
    are converted to that type and the output has it.  np.float32 runs the Float32 kernel (both products on the Float32 matrix
    instruction, the sum over the columns of K in Float64 across windows of 128): kernel values to about 1e-6 of the variance.
    block=128 takes the columns of V 128 at a time through the wide kernel (agp_kernel_matmul_wide, csrc/agp_kmv_wide.h): every
    kernel tile is computed once for 128 columns, not once per 32, and each column equals block=32's bit for bit.  Float64 only.
    65 <= D <= 128 goes through agp_kernel_matmul_hd (csrc/agp_kmv_hd.h), Float64 in blocks of 32 columns: dtype=np.float32 and
    block=128 are refused there."""
    if Y is not None and diag_add != 0.0:
        raise ValueError("diag_add is added to the diagonal of K(X, X): it needs Y=None")
    dtype = _np_dtype(dtype, "dtype")
    block = _block(block, "kernel_matmul")
    D = 1 if np.ndim(X) == 1 else np.shape(X)[1]
    if dtype is np.float32:
        _refuse_hd(D, "kernel_matmul", "dtype=np.float32 (the Float32 kernel)", ValueError)
    if block == WIDE:
        _refuse_hd(D, "kernel_matmul", "block=128 (the wide kernel)", ValueError)
    torch = _torch()
    cx = _Ctx(device)
    try:
        vec = np.ndim(V) == 1
        out = _kernel_matmul(cx, kernel, cx.dev_tensor(X, dtype), cx.dev_tensor(V, dtype),
                             None if Y is None else cx.dev_tensor(Y, dtype), diag_add, col_groups, dtype, block)
    finally:
        cx.close()
    if vec:
        out = out[:, 0]
    return out if isinstance(V, torch.Tensor) else out.cpu().numpy()


def _bilinear_grad(cx, kernel, Xd, Ud, Vd, w, col_groups=0):
    """(dvariance, dscales[D]) of sum_c w_c Ud[:, c]' K(Xd, Xd) Vd[:, c]; blocks of 32 columns, added in order"""
    if kernel._kind == capi.K_EXPONENTIAL:
        raise NotImplementedError("kernel_bilinear_grad: the ExponentialKernel has no derivative at coincident points; "
                                  "SqExponentialKernel, Matern32Kernel and Matern52Kernel only")
    Xd, Ud, Vd = _rows(Xd), _rows(Ud), _rows(Vd)
    n, D = Xd.shape
    if Ud.shape != Vd.shape or Ud.shape[0] != n:
        raise ValueError(f"U {tuple(Ud.shape)} and V {tuple(Vd.shape)} must both be {n} x r")
    w = np.ones(Ud.shape[1]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    if len(w) != Ud.shape[1]:
        raise ValueError(f"{len(w)} weights for {Ud.shape[1]} pairs")
    kd, keep = kernel.desc(D)
    dvar, dsc = 0.0, np.zeros(D)
    for c0 in range(0, Ud.shape[1], MAXR):
        u, v = Ud[:, c0:c0 + MAXR], Vd[:, c0:c0 + MAXR]
        r = u.shape[1]
        o1, oD = C.c_double(), (C.c_double * D)()
        cx.chk(capi.lib().agp_kernel_bilinear_grad(cx.ctx, capi.F64, C.byref(kd), C.c_void_p(Xd.data_ptr()), n, Xd.stride(0), D,
                                                   C.c_void_p(u.data_ptr()), Ud.stride(0), C.c_void_p(v.data_ptr()), Vd.stride(0), r,
                                                   (C.c_double * r)(*w[c0:c0 + r]), int(col_groups), C.byref(o1), oD))
        dvar += o1.value
        dsc += np.array(oD)
    del keep
    return dvar, dsc


def kernel_bilinear_grad(kernel, X, U, V, w=None, col_groups: int = 0, device: Optional[int] = None):
    """(dvariance, dscales[D]): the derivatives of sum_c w_c U[:, c]' K(X, X) V[:, c] with respect to the kernel's variance and to the
    scale of each input dimension (an isotropic kernel's is their sum), on the device with neither K nor sum_c w_c u_c v_c' formed.
    X: n x D, U and V: n x r (vectors count as n x 1), w: r weights (default 1).  More than 32 pairs are taken in blocks of 32 and added
    in order.  Two calls agree bit for bit.  The ExponentialKernel is refused.  col_groups as in kernel_matmul."""
    cx = _Ctx(device)
    try:
        return _bilinear_grad(cx, kernel, cx.dev_tensor(X), cx.dev_tensor(U), cx.dev_tensor(V), w, col_groups)
    finally:
        cx.close()


def _refuse_exponential(kernel, who):
    if kernel._kind == capi.K_EXPONENTIAL:
        raise NotImplementedError(f"{who}: the ExponentialKernel has no derivative at coincident points; "
                                  "SqExponentialKernel, Matern32Kernel and Matern52Kernel only")


def _matmul_dx_blocks(call, Xd, Vd, D, paired):
    """the blocks of 32 of agp_kernel_matmul_dx / agp_gp_cg_apply_dx: columns of V in shared mode -> (n, r, D), rows of X with their
    own columns of V in paired mode -> (n, D).  call(x, v, r, paired, out) launches one block."""
    torch = _torch()
    n, r = Xd.shape[0], Vd.shape[1]
    if paired:
        if r != n:
            raise ValueError(f"paired: V needs one column per row of X ({n}), got {r}")
        out = torch.empty(n, D, dtype=torch.float64, device=Xd.device)
        for i0 in range(0, n, MAXR):
            call(Xd[i0:i0 + MAXR], Vd[:, i0:i0 + MAXR], min(MAXR, n - i0), 1, out[i0:i0 + MAXR])
        return out
    out = torch.empty(n, r, D, dtype=torch.float64, device=Xd.device)
    for c0 in range(0, r, MAXR):
        call(Xd, Vd[:, c0:c0 + MAXR], min(MAXR, r - c0), 0, out[:, c0:c0 + MAXR])
    return out


def _kernel_matmul_grad(cx, kernel, Xd, Vd, Yd, paired, col_groups):
    _refuse_exponential(kernel, "kernel_matmul_grad")
    Xd, Vd, Yd = _rows(Xd), _rows(Vd), _rows(Yd)
    n, D = Xd.shape
    p = Yd.shape[0]
    if Vd.shape[0] != p:
        raise ValueError(f"V has {Vd.shape[0]} rows, K(X, Y) has {p} columns")
    kd, keep = kernel.desc(D)

    def call(x, v, r, prd, o):
        cx.chk(capi.lib().agp_kernel_matmul_dx(cx.ctx, capi.F64, C.byref(kd), C.c_void_p(x.data_ptr()), x.shape[0], Xd.stride(0),
                                               C.c_void_p(Yd.data_ptr()), p, Yd.stride(0), D, C.c_void_p(v.data_ptr()), Vd.stride(0),
                                               r, prd, int(col_groups), C.c_void_p(o.data_ptr()), o.stride(0)))

    out = _matmul_dx_blocks(call, Xd, Vd, D, paired)
    del keep
    return out


def kernel_matmul_grad(kernel, X, V, Y, paired: bool = False, col_groups: int = 0, device: Optional[int] = None):
    """The derivative of K(X, Y) V with respect to the rows of X, on the device with neither K nor its n x p x D derivative formed
    (agp_kernel_matmul_dx, csrc/agp_kmv_dx.h).  X: n x D, Y: p x D, V: p x r.
    paired=False: out[i, c, d] = d/dX[i, d] of (K(X, Y) V)[i, c], shape (n, r, D); (n, D) for a vector V.
    paired=True:  V is p x n and out[i, d] = d/dX[i, d] of K(X[i], Y) V[:, i] with V held fixed, shape (n, D).
    More than 32 columns -- in paired mode more than 32 rows -- are taken in blocks of 32.  Float64, D <= 64; a row of X that equals a
    row of Y is an ordinary input.  Two calls agree bit for bit, and without `paired` an output column depends on its own column of V
    only.  The ExponentialKernel is refused.  col_groups as in kernel_matmul.  Arrays in, a NumPy array out; device tensors in, a device
    tensor out."""
    torch = _torch()
    cx = _Ctx(device)
    try:
        vec = np.ndim(V) == 1
        out = _kernel_matmul_grad(cx, kernel, cx.dev_tensor(X), cx.dev_tensor(V), cx.dev_tensor(Y), bool(paired), col_groups)
    finally:
        cx.close()
    if vec and not paired:
        out = out[:, 0]
    return out if isinstance(V, torch.Tensor) else out.cpu().numpy()


class IterativeGP:
    """IterativeGP(X, y, kernel; noise=1e-5, mean=None, tol=1e-8, max_iter=1000, precond_rank=64): the exact GP posterior at FIXED
    hyper-parameters.  alpha = (K + noise I)^-1 (y - mean) is solved on first use by preconditioned CG on the matrix-free operator;
    nothing of size N x N is ever stored.  The preconditioner is a pivoted partial Cholesky of K of rank `precond_rank` (0: none).
    precond_rank and max_iter are interface defaults, not tuned.  mean: None, a constant, or one value per training point.

    predict_f(model, Xt, cov=True) -> (mean, variance): the mean is one operator product; the variance costs ONE BATCHED CG RUN PER 32
    TEST POINTS (k** - k*' (K + noise I)^-1 k*), so ask for it on as many points as are needed and no more.  block=128: solve,
    operator, the variance loops of predict_f / predict_y / predict_f_grad, log_marginal_likelihood, optimize and the solve of
    sample_paths take 128 columns per CG run on the wide operator kernel (csrc/agp_kmv_wide.h), which computes every kernel tile
    once for all of them; each column's CG recurrence is unchanged, and the Float32 operator is refused with it.  predict_y adds the
    noise.  model.solve(B) exposes the solver, model.info what the last solve did.  log_marginal_likelihood (also ELBO(model)) and
    optimize learn the kernel and the noise; there is no train_.

    operator_dtype=np.float32 runs every operator product of the CG -- in solve, alpha, predict_f, log_marginal_likelihood and
    optimize alike -- on the Float32 kernel; the CG's vectors and reductions, the preconditioner, the probes and the gradient kernel
    stay Float64.  The Float32 operator is a slightly different, FIXED linear map (kernel values to about 1e-6 of the variance): CG
    solves THAT system, and its recursive residual stops tracking the true one somewhere around the operator's own error.  A `tol`
    below that level shows up as converged = False in model.info; it is not an exception.  The option is meant for
    log_marginal_likelihood and optimize, whose Monte-Carlo error is orders of magnitude larger; the default, and any prediction that
    must be exact, stays np.float64.  No iterative refinement is built.

    D <= 128.  With 65 <= D <= 128 every operator product runs on the kernel for that range (csrc/agp_kmv_hd.h): solve, operator,
    alpha, predict_f, predict_y, log_marginal_likelihood(grad=False) and ELBO(model) are served; operator_dtype=np.float32 and
    block=128 (ValueError), log_marginal_likelihood(grad=True), optimize, predict_f_grad and sample_paths (NotImplementedError) are
    not: their kernels stop at D = 64."""

    def __init__(self, X, y, kernel, *, noise: float = 1e-5, mean=None, tol: float = 1e-8, max_iter: int = 1000,
                 precond_rank: int = 64, check_every: int = 10, device: Optional[int] = None, operator_dtype=np.float64,
                 block: int = 32):
        X = np.asarray(X, dtype=np.float64)
        X = np.ascontiguousarray(X[:, None] if X.ndim == 1 else X)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if len(y) != X.shape[0]:
            raise ValueError(f"There is not the same number of samples in X ({X.shape[0]}) and y ({len(y)})")
        if not noise > 0:
            raise ValueError("noise must be positive")
        if mean is not None and not np.isscalar(mean) and len(mean) != X.shape[0]:
            raise ValueError("a mean vector needs one value per training point")
        self.X, self.y, self.kernel, self.noise, self.mean = X, y, copy.deepcopy(kernel), float(noise), mean
        self.tol, self.max_iter, self.precond_rank, self.check_every = float(tol), int(max_iter), int(precond_rank), int(check_every)
        self.N, self.D = X.shape
        self.operator_dtype = _np_dtype(operator_dtype, "operator_dtype")
        self.block = _block(block, "IterativeGP")
        if self.block == WIDE and self.operator_dtype is np.float32:
            raise ValueError("IterativeGP: block=128 needs operator_dtype=np.float64 (no Float32 wide block is built)")
        if self.operator_dtype is np.float32:
            _refuse_hd(self.D, "IterativeGP", "operator_dtype=np.float32 (the Float32 operator)", ValueError)
        if self.block == WIDE:
            _refuse_hd(self.D, "IterativeGP", "block=128 (the wide kernel)", ValueError)
        self.device = device
        self.info = None
        self.rank_used = None
        self.seed = None  # of sample_paths(model, ...; seed=None): drawn once, kept
        self._cx = self._h = self._Xd = self._alpha = None

    @classmethod
    def from_model(cls, m, X, y, **kwargs):
        """kernel, noise and prior mean of a trained GP or Gaussian-likelihood SVGP, on the data (X, y)"""
        if not isinstance(getattr(m, "likelihood", None), GaussianLikelihood) or getattr(m, "n_latent", 1) != 1:
            raise ValueError("IterativeGP.from_model takes a GP or an SVGP with a Gaussian likelihood")
        mean = m.mean
        if mean is not None and not np.isscalar(mean) and len(mean) != len(np.asarray(X)):
            raise ValueError("the model's prior mean is a vector over other points: pass mean= explicitly")
        kwargs.setdefault("mean", mean)
        kwargs.setdefault("noise", m.likelihood.sigma2)
        return cls(X, y, m.kernels[0], **kwargs)

    # ---- device side ----
    def _solver(self):
        if self._h is None:
            self._cx = _Ctx(self.device)
            self._Xd = self._cx.dev_tensor(self.X)
            kd, keep = self.kernel.desc(self.D)
            h, used = C.c_void_p(), C.c_int64()
            self._cx.chk(capi.lib().agp_gp_cg_create(self._cx.ctx, C.byref(kd), C.c_void_p(self._Xd.data_ptr()), self.N,
                                                     self._Xd.stride(0), self.D, self.noise, self.precond_rank, C.byref(h),
                                                     C.byref(used)))
            del keep
            self._h, self.rank_used = h, int(used.value)
            if self.operator_dtype is np.float32:
                self._cx.chk(capi.lib().agp_gp_cg_set_operator_dtype(h, capi.F32))
            if self.block != MAXR:
                try:
                    self._cx.chk(capi.lib().agp_gp_cg_set_block(h, self.block))
                except Exception:
                    self.close()  # the handle is still valid at 32 columns, but not the one this model asked for: the next use builds anew
                    raise
        return self._h

    def _solve_dev(self, Bd, tol, max_iter):
        """(K + noise I)^-1 B for a device tensor B (n x r, any r), with the per-column report"""
        torch = _torch()
        h = self._solver()
        Bd = _rows(Bd)
        A = torch.empty(Bd.shape, dtype=torch.float64, device=self._cx.dev)
        its, res, conv = [], [], []
        for c0 in range(0, Bd.shape[1], self.block):
            b, a = Bd[:, c0:c0 + self.block], A[:, c0:c0 + self.block]
            r = b.shape[1]
            it, rr, cv = (C.c_int32 * r)(), (C.c_double * r)(), (C.c_int32 * r)()
            self._cx.chk(capi.lib().agp_gp_cg_solve(h, C.c_void_p(b.data_ptr()), Bd.stride(0), r, tol, max_iter, self.check_every,
                                                    C.c_void_p(a.data_ptr()), A.stride(0), it, rr, cv))
            its += list(it)
            res += list(rr)
            conv += [bool(v) for v in cv]
        self.info = dict(iterations=np.array(its), residuals=np.array(res), converged=np.array(conv), rank_used=self.rank_used)
        return A

    def solve(self, B, tol: Optional[float] = None, max_iter: Optional[int] = None):
        """(K(X, X) + noise I)^-1 B, B of N rows; what the solve did is in model.info (iterations, residuals = final |r| / |b|,
        converged, per column).  Reaching max_iter is reported there, not raised."""
        torch = _torch()
        self._solver()
        vec = np.ndim(B) == 1
        Bd = self._cx.dev_tensor(B)
        if Bd.shape[0] != self.N:
            raise ValueError(f"B has {Bd.shape[0]} rows, the model {self.N} points")
        A = self._solve_dev(Bd, self.tol if tol is None else float(tol), self.max_iter if max_iter is None else int(max_iter))
        A = A[:, 0] if vec else A
        return A if isinstance(B, torch.Tensor) else A.cpu().numpy()

    def operator(self, V):
        """(K(X, X) + noise I) V on the operator the solves run on (operator_dtype), V of N rows: the system CG solves"""
        torch = _torch()
        h = self._solver()
        vec = np.ndim(V) == 1
        Vd = _rows(self._cx.dev_tensor(V))
        if Vd.shape[0] != self.N:
            raise ValueError(f"V has {Vd.shape[0]} rows, the model {self.N} points")
        out = torch.empty(Vd.shape, dtype=torch.float64, device=self._cx.dev)
        for c0 in range(0, Vd.shape[1], self.block):
            v, o = Vd[:, c0:c0 + self.block], out[:, c0:c0 + self.block]
            self._cx.chk(capi.lib().agp_gp_cg_apply(h, C.c_void_p(v.data_ptr()), Vd.stride(0), v.shape[1], C.c_void_p(o.data_ptr()),
                                                    out.stride(0)))
        out = out[:, 0] if vec else out
        return out if isinstance(V, torch.Tensor) else out.cpu().numpy()

    def _mu0(self, n):
        return 0.0 if self.mean is None else float(self.mean) if np.isscalar(self.mean) else np.asarray(self.mean, dtype=np.float64)

    def alpha(self):
        """(K + noise I)^-1 (y - mean), on the device (solved once)"""
        if self._alpha is None:
            self._solver()
            self._alpha = self._solve_dev(self._cx.dev_tensor(self.y - self._mu0(self.N)), self.tol, self.max_iter)
            self.alpha_info = self.info
        return self._alpha

    # ---- log marginal likelihood ----
    def log_marginal_likelihood(self, num_probes: int = 32, seed: int = 0, base_samples=None, grad: bool = False, _t0: int = 0):
        """log p(y) = -1/2 (y - mean)' alpha - 1/2 log det(K + noise I) - N/2 log 2 pi with the log-determinant estimated as
        log det P + (1/t) sum_c (z_c' P^-1 z_c) e1' log(T_c) e1 over t probes z_c ~ N(0, P) (P: the preconditioner, T_c: the Lanczos
        tridiagonal of probe c from its CG coefficients); one batched CG per 32 columns of [y - mean, probes].  The probes come from
        `seed` (two calls agree bit for bit) or from base_samples, t x (N + rank_used) standard normals (sqrt(t) I makes the
        estimators exact traces).  grad=True: (value, dict(variance=, scales=[D], noise=)) -- derivatives with respect to the
        kernel's variance, the per-dimension scales (for a ScaleTransform also scale= their sum) and the noise, the trace terms by
        the same probes.  num_probes is an interface default, not tuned; accuracy is set by it, by tol and by max_iter."""
        if grad:
            _refuse_hd(self.D, "IterativeGP.log_marginal_likelihood(grad=True)", "the derivative bilinear form (csrc/agp_kmv_grad.h)")
        torch = _torch()
        L = capi.lib()
        h = self._solver()
        cx, n = self._cx, self.N
        base = None
        if base_samples is not None:
            base = _rows(cx.dev_tensor(np.asarray(base_samples, dtype=np.float64)))
            if base.shape[1] != n + self.rank_used:
                raise ValueError(f"base_samples needs {n + self.rank_used} columns (N + rank_used), got {base.shape[1]}")
        t = int(num_probes) if base is None else base.shape[0]
        if t < 1:
            raise ValueError("num_probes must be positive")
        B = torch.empty(n, 1 + t, dtype=torch.float64, device=cx.dev)
        B[:, 0] = cx.dev_tensor(self.y - self._mu0(n))[:, 0]
        Z = B[:, 1:]
        cx.chk(L.agp_gp_cg_probes(h, t, None if base is None else C.c_void_p(base.data_ptr()), 0 if base is None else base.stride(0),
                                  int(seed), int(_t0), C.c_void_p(Z.data_ptr()), B.stride(0)))
        A, Z0 = torch.empty_like(B), torch.empty_like(B)
        its, res, conv, bpb, quad = [], [], [], [], []
        for c0 in range(0, 1 + t, self.block):
            b, a, z0 = B[:, c0:c0 + self.block], A[:, c0:c0 + self.block], Z0[:, c0:c0 + self.block]
            r = b.shape[1]
            it, rr, cv, pb, qd = (C.c_int32 * r)(), (C.c_double * r)(), (C.c_int32 * r)(), (C.c_double * r)(), (C.c_double * r)()
            cx.chk(L.agp_gp_cg_solve_slq(h, C.c_void_p(b.data_ptr()), B.stride(0), r, self.tol, self.max_iter, self.check_every,
                                         C.c_void_p(a.data_ptr()), A.stride(0), C.c_void_p(z0.data_ptr()), Z0.stride(0), it, rr, cv,
                                         pb, qd))
            its, res, conv, bpb, quad = its + list(it), res + list(rr), conv + [bool(v) for v in cv], bpb + list(pb), quad + list(qd)
        self.info = dict(iterations=np.array(its), residuals=np.array(res), converged=np.array(conv), rank_used=self.rank_used)
        if self._alpha is None:
            self._alpha, self.alpha_info = A[:, :1].clone(), self.info
        ldp = C.c_double()
        cx.chk(L.agp_gp_cg_precond_logdet(h, C.byref(ldp)))
        logdet = ldp.value + float(np.dot(bpb[1:], quad[1:])) / t
        value = -0.5 * float(B[:, 0] @ A[:, 0]) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
        if not grad:
            return value
        V = torch.cat([A[:, :1], Z0[:, 1:]], dim=1)
        w = np.concatenate([[0.5], np.full(t, -0.5 / t)])
        dvar, dsc = _bilinear_grad(cx, self.kernel, self._Xd, A, V, w)
        dnoise = float((torch.as_tensor(w, device=cx.dev) * (A * V).sum(dim=0)).sum())
        g = dict(variance=dvar, scales=dsc, noise=dnoise)
        if not hasattr(self.kernel.transform, "v"):
            g["scale"] = float(dsc.sum())
        return value, g

    def optimize(self, iterations: int, optimiser=None, opt_noise: bool = True, num_probes: int = 32, seed: int = 0,
                 base_samples=None):
        """`iterations` ADAM ascent steps (optimiser=ADAM(0.01)) on the stochastic log marginal likelihood, in the logarithms of the
        kernel's variance (if it has one: `a * k`), its scale or ARD scales (if it has a transform) and, with opt_noise, the noise --
        at most D + 2 scalars, stepped on the host.  The solver is rebuilt after every step (its preconditioner depends on the
        kernel) and every step draws a fresh probe table from (seed, iteration).  num_probes and the step size are interface
        defaults, not tuned.  Returns the values log p(y) at the parameters BEFORE each step."""
        from .kernels import ARDTransform, ScaleTransform

        _refuse_hd(self.D, "IterativeGP.optimize", "the derivative bilinear form of its gradient (csrc/agp_kmv_grad.h)")
        o = ADAM(0.01) if optimiser is None else optimiser
        if not isinstance(o, ADAM):
            raise TypeError("IterativeGP.optimize takes an ADAM optimiser")
        k = self.kernel
        ard = isinstance(k.transform, ARDTransform)
        nsc = 0 if k.transform is None else (self.D if ard else 1)
        m, v, trace = np.zeros(2 + nsc), np.zeros(2 + nsc), []
        for it in range(int(iterations)):
            val, g = self.log_marginal_likelihood(num_probes, seed, base_samples, grad=True, _t0=it * int(num_probes))
            trace.append(val)
            sc = k.scales(self.D)[:nsc] if nsc else np.zeros(0)
            theta = np.concatenate([[k.variance], sc, [self.noise]])
            dth = np.concatenate([[g["variance"] if k.has_variance else 0.0], g["scales"] if ard else [g["scale"]] * nsc,
                                  [g["noise"] if opt_noise else 0.0]])
            gl = theta * dth  # d / d log theta
            m = o.beta[0] * m + (1 - o.beta[0]) * gl
            v = o.beta[1] * v + (1 - o.beta[1]) * gl * gl
            step = o.eta * (m / (1 - o.beta[0] ** (it + 1))) / (np.sqrt(v / (1 - o.beta[1] ** (it + 1))) + o.eps)
            theta = theta * np.exp(step)
            k.variance, self.noise = float(theta[0]), float(theta[-1])
            if nsc:
                k.transform = ARDTransform(theta[1:-1]) if ard else ScaleTransform(float(theta[1]))
            self.close()  # the handle belongs to the old kernel and noise
            self._alpha = None
        return np.array(trace)

    def close(self):
        if self._h is not None:
            capi.lib().agp_gp_cg_destroy(self._h)
            self._h = None
        if self._cx is not None:
            self._cx.close()
            self._cx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return f"Iterative exact Gaussian Process on {self.N} points (noise {self.noise:g})"


@predict_f.register(IterativeGP)
def _predict_f_iterative(model: IterativeGP, X_test, state=None, *, cov: bool = True, diag: bool = True, obsdim: int = 1):
    """(mean, variance) of the latent at X_test, or the mean alone with cov=False.  The variance costs one batched CG run per 32 test
    points.  diag=False (the full predictive covariance) is not built."""
    if not diag:
        raise NotImplementedError("IterativeGP.predict_f: diag=False (the full predictive covariance) is not built")
    torch = _torch()
    alpha = model.alpha()
    cx = model._cx
    Xt = _test_points(model, X_test, obsdim)
    mu0 = 0.0 if model.mean is None or not np.isscalar(model.mean) else float(model.mean)  # (a vector mean lives on the training points)
    mean = (_kernel_matmul(cx, model.kernel, Xt, alpha, model._Xd, 0.0, 0)[:, 0] + mu0).cpu().numpy()
    if not cov:
        return mean
    nt, variance = Xt.shape[0], model.kernel.desc(model.D)[0].variance
    var = torch.empty(nt, dtype=torch.float64, device=cx.dev)
    for c0 in range(0, nt, model.block):
        ks, sol = _kstar_solve(model, Xt[c0:c0 + model.block])
        var[c0:c0 + model.block] = variance - (ks * sol).sum(dim=0)
    return mean, var.cpu().numpy()


def _kstar_solve(model, xt):
    """(K(X, xt), (K + noise I)^-1 K(X, xt)) for a chunk of at most model.block test points (rows of a device tensor): one batched CG"""
    cx = model._cx
    kd, keep = model.kernel.desc(model.D)
    ks = _torch().empty(model.N, xt.shape[0], dtype=_torch().float64, device=cx.dev)
    cx.chk(capi.lib().agp_kernelmatrix(cx.ctx, capi.F64, C.byref(kd), C.c_void_p(model._Xd.data_ptr()), model.N, model._Xd.stride(0),
                                       None, C.c_void_p(xt.data_ptr()), xt.shape[0], xt.stride(0), model.D,
                                       C.c_void_p(ks.data_ptr()), ks.stride(0)))
    del keep
    return ks, model._solve_dev(ks, model.tol, model.max_iter)


def _test_points(model, X_test, obsdim):
    Xt = model._cx.dev_tensor(np.asarray(X_test, dtype=np.float64))
    if obsdim == 2:  # (a fresh tensor: a single point transposed would keep a row pitch of 1)
        Xt = _torch().empty(Xt.shape[1], Xt.shape[0], dtype=Xt.dtype, device=Xt.device).copy_(Xt.t())
    if Xt.shape[1] != model.D:
        raise ValueError(f"X_test has {Xt.shape[1]} dimensions, the model {model.D}")
    return Xt


def predict_f_grad_iterative(model: IterativeGP, X_test, *, cov: bool = True, obsdim: int = 1):
    """(dmu, dvar), (n_t, D) arrays: the gradients of predict_f(model, X_test) with respect to the test inputs; dmu alone with
    cov=False, which runs no solve beyond alpha.  dmu = d/dx* K(x*, X) alpha is one launch of the fused derivative operator
    (agp_gp_cg_apply_dx on the handle's prepared training side); dvar = -2 (d/dx* K(x*, X)) (K + noise I)^-1 K(X, x*) is its paired
    mode on the solutions predict_f's variance needs anyway: it costs ONE BATCHED CG RUN PER 32 TEST POINTS.  A prior mean (a
    constant, or one value per training point) contributes nothing.  With operator_dtype=np.float32 the solves run on the Float32
    operator; the gradient kernel is Float64."""
    if not isinstance(cov, bool):
        raise TypeError("predict_f_grad: cov is a bool")
    if obsdim not in (1, 2):
        raise ValueError("predict_f_grad: obsdim is 1 (points are rows) or 2 (points are columns)")
    _refuse_exponential(model.kernel, "predict_f_grad")
    _refuse_hd(model.D, "predict_f_grad(IterativeGP)", "the derivative operator (csrc/agp_kmv_dx.h)")
    alpha = model.alpha()
    cx, h, D = model._cx, model._solver(), model.D
    Xt = _rows(_test_points(model, X_test, obsdim))

    def call(x, v, r, prd, o):
        cx.chk(capi.lib().agp_gp_cg_apply_dx(h, C.c_void_p(x.data_ptr()), x.shape[0], x.stride(0), C.c_void_p(v.data_ptr()),
                                             v.stride(0), r, prd, C.c_void_p(o.data_ptr()), o.stride(0)))

    dmu = _matmul_dx_blocks(call, Xt, _rows(alpha), D, False)[:, 0].cpu().numpy()
    if not cov:
        return dmu
    dvar = _torch().empty(Xt.shape[0], D, dtype=_torch().float64, device=cx.dev)
    for c0 in range(0, Xt.shape[0], model.block):  # (one solve per block of the model; the derivative operator still 32 at a time)
        xt = Xt[c0:c0 + model.block]
        dvar[c0:c0 + model.block] = -2.0 * _matmul_dx_blocks(call, xt, _kstar_solve(model, xt)[1], D, True)
    return dmu, dvar.cpu().numpy()


@predict_y.register(IterativeGP)
def _predict_y_iterative(model: IterativeGP, X_test, state=None, *, cov: bool = True, obsdim: int = 1):
    """predict_f with the noise added to the variance"""
    out = predict_f(model, X_test, cov=cov, obsdim=obsdim)
    return (out[0], out[1] + model.noise) if cov else out


@train_.register(IterativeGP)
def _train_iterative(model: IterativeGP, *args, **kwargs):
    raise NotImplementedError("IterativeGP has no train_: it is the posterior at fixed hyper-parameters (the log marginal likelihood "
                              "needs a log-determinant this path does not form).  Learn them with GP or SVGP, then "
                              "IterativeGP.from_model(m, X, y)")


@ELBO.register(IterativeGP)
def _elbo_iterative(model: IterativeGP, *args, num_probes: int = 32, seed: int = 0, **kwargs) -> float:
    """ELBO(model) of an IterativeGP: its (stochastic) log marginal likelihood"""
    return model.log_marginal_likelihood(num_probes=num_probes, seed=seed)
