"""Synthetic benchmark problems of SURVEY.md 8(d): r(x) = A tanh(x) - b, J = A diag(1 - tanh(x)^2).

Inputs come from the counter-based generator inside liblsqhip.so (host code), so the CPU baseline
and every GPU rank regenerate bit-identical problems from the seed alone.  f!/g! run on the device
(lsq_model_*), so nothing crosses PCIe inside the timed loop.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import (DeviceVector, LeastSquaresResult, _run_native, _run_native_batched, default_context)

BASE_SEED = 20260928


def sparse_inputs(m, n, per_col, seed):
    """CSC pattern/values with exactly per_col sorted distinct rows per column (nnz = n*per_col)."""
    nnz = n * per_col
    colptr = np.zeros(n + 1, dtype=np.int32)
    rowval = np.zeros(nnz, dtype=np.int32)
    nzval = np.zeros(nnz)
    check(lib().lsq_synth_sparse(m, n, per_col, seed, colptr.ctypes.data_as(_lib.c_ip),
                                 rowval.ctypes.data_as(_lib.c_ip), nzval.ctypes.data_as(_lib.c_dp)))
    return colptr, rowval, nzval


def dense_inputs(m, n, seed):
    v = np.zeros(m * n)
    check(lib().lsq_synth_dense(m, n, seed, v.ctypes.data_as(_lib.c_dp)))
    return v


def blockdiag_inputs(nblocks, mb, nb, seed):
    """Values of blkdiag(A_1 .. A_B) in [block][column][row] order: the dense generator's mb x (B*nb) matrix, column-major --
    every entry N(0,1)/sqrt(mb), block b = its columns b*nb .. (b+1)*nb - 1."""
    return dense_inputs(mb, nblocks * nb, seed)


def bordered_inputs(nblocks, mb, nb, ng, seed):
    """Values of [blkdiag(A_1 .. A_B) | C] in the order of a BorderedBlockDiagonal's `.data`: the blocks as blockdiag_inputs
    draws them, then the border -- the dense generator's m x ng matrix (m = B*mb) at seed + 1, column-major, every entry
    N(0,1)/sqrt(m)."""
    return np.concatenate([blockdiag_inputs(nblocks, mb, nb, seed), dense_inputs(nblocks * mb, ng, seed + 1)])


def uniform(n, seed, lo=-1.0, hi=1.0):
    v = np.zeros(n)
    check(lib().lsq_synth_uniform(n, seed, lo, hi, v.ctypes.data_as(_lib.c_dp)))
    return v


def normal(n, seed):
    v = np.zeros(n)
    check(lib().lsq_synth_normal(n, seed, v.ctypes.data_as(_lib.c_dp)))
    return v


def rhs_for(matvec, m, n, seed, noise=1e-3):
    """b = A tanh(x_true) + noise * N(0,1), x_true ~ U(-1,1)."""
    x_true = uniform(n, seed + 101)
    b = matvec(np.tanh(x_true)) + noise * normal(m, seed + 202)
    return x_true, b


def csc_matvec(m, colptr, rowval, nzval, t):
    """Host A*t for building b (numpy, vectorised)."""
    n = len(colptr) - 1
    cols = np.repeat(np.arange(n), np.diff(colptr))
    return np.bincount(rowval, weights=nzval * t[cols], minlength=m)


class _Handle:      # minimal handle wrapper for _run_native
    __slots__ = ("h",)

    def __init__(self, h):
        self.h = h


class TanhProblem:
    """Device-resident problem: Jacobian handle + model (A, b) + x / fcur vectors."""

    def __init__(self, m, n, sparse=True, per_col=None, seed=BASE_SEED, ctx=None, inputs=None, b=None, blockdiag=None,
                 bordered=None):
        """blockdiag=(nblocks, mb, nb): A = blkdiag of nblocks dense mb x nb blocks (m = nblocks*mb, n = nblocks*nb) on a
        block-diagonal handle (lsq_blockdiag_create); `inputs` / self.A are then the values in [block][column][row] order.
        bordered=(nblocks, mb, nb, ng): A = [blkdiag | C] with ng shared columns (m = nblocks*mb, n = nblocks*nb + ng) on a
        bordered handle (lsq_blockdiag_bordered_create); `inputs` / self.A are the values in bordered_inputs' order."""
        self.ctx = ctx or default_context()
        self.m, self.n, self.sparse = m, n, sparse
        self.blockdiag = None
        self.bordered = None
        L = lib()
        h = C.c_void_p()
        if bordered is not None:
            B, mb, nb, ng = (int(v) for v in bordered)
            if (m, n) != (B * mb, B * nb + ng):
                raise ValueError("bordered=(%d, %d, %d, %d) is a %d x %d problem, not %d x %d"
                                 % (B, mb, nb, ng, B * mb, B * nb + ng, m, n))
            self.bordered, self.sparse = (B, mb, nb, ng), True
            if inputs is None:
                inputs = bordered_inputs(B, mb, nb, ng, seed)
            self.A = inputs
            check(L.lsq_blockdiag_bordered_create(self.ctx.h, B, mb, nb, ng, C.byref(h)))
            self.nnz = len(self.A)
            A3 = self.A[:B * mb * nb].reshape((B, nb, mb))
            Cg = self.A[B * mb * nb:].reshape((m, ng), order="F")
            mv = lambda t: np.einsum("bjr,bj->br", A3, t[:B * nb].reshape((B, nb))).reshape(-1) + Cg @ t[B * nb:]
        elif blockdiag is not None:
            B, mb, nb = (int(v) for v in blockdiag)
            if (m, n) != (B * mb, B * nb):
                raise ValueError("blockdiag=(%d, %d, %d) is a %d x %d problem, not %d x %d" % (B, mb, nb, B * mb, B * nb, m, n))
            self.blockdiag, self.sparse = (B, mb, nb), True
            if inputs is None:
                inputs = blockdiag_inputs(B, mb, nb, seed)
            self.A = inputs
            check(L.lsq_blockdiag_create(self.ctx.h, B, mb, nb, C.byref(h)))
            self.nnz = len(self.A)
            A3 = self.A.reshape((B, nb, mb))
            mv = lambda t: np.einsum("bjr,bj->br", A3, t.reshape((B, nb))).reshape(-1)
        elif sparse:
            if inputs is None:
                inputs = sparse_inputs(m, n, per_col, seed)
            colptr, rowval, nzval = inputs
            self.colptr, self.rowval, self.A = colptr, rowval, nzval
            check(L.lsq_csc_create(self.ctx.h, m, n, colptr.ctypes.data_as(_lib.c_ip),
                                   rowval.ctypes.data_as(_lib.c_ip), C.byref(h)))
            self.nnz = len(nzval)
            mv = lambda t: csc_matvec(m, colptr, rowval, nzval, t)
        else:
            if inputs is None:
                inputs = dense_inputs(m, n, seed)
            self.A = inputs
            check(L.lsq_dense_create(self.ctx.h, m, n, C.byref(h)))
            self.nnz = m * n
            Amat = self.A.reshape((m, n), order="F")
            mv = lambda t: Amat @ t
        self.J = h
        if b is None:
            self.x_true, self.b = rhs_for(mv, m, n, seed)
        else:                       # (a row block of a larger problem: the caller owns the right-hand side)
            self.x_true, self.b = None, np.ascontiguousarray(b, dtype=np.float64)
        md = C.c_void_p()
        check(L.lsq_model_tanh_create(self.ctx.h, self.J, self.A.ctypes.data_as(_lib.c_dp),
                                      self.b.ctypes.data_as(_lib.c_dp), C.byref(md)))
        self.model = md
        self.x = DeviceVector(self.ctx, n)
        self.fcur = DeviceVector(self.ctx, m)
        self._Jd = None
        self._fg = None

    def reset(self, x0=None):
        if x0 is None:      # x <- 0 on the device (a fill kernel in stream order: no host buffer, no blocking copy)
            check(lib().lsq_fill(self.ctx.h, self.n, 0.0, self.x.ptr))
        else:
            self.x.set(x0)

    def optimize(self, optimizer_kind, solver_kind, x_tol=1e-8, f_tol=1e-8, g_tol=1e-8, iterations=1000,
                 delta=None, trace=False, allreduce=None, fetch_x=True, row_allreduce=None, row_allreduce_user=None,
                 global_rows=0, lower=None, upper=None):
        """lower / upper: box bounds of length n (host arrays), as optimize_ takes them; None = unbounded."""
        # (the handle wrapper and the two callback pointers are made once per problem: a solve of the bench schedule takes 2 ms,
        #  and tens of microseconds of interpreter work per call showed in its timeline)
        if self._Jd is None:
            L = lib()
            self._Jd = _Handle(self.J)
            self._fg = (L.lsq_model_f(), L.lsq_model_g())
        Jd = self._Jd
        st, res, tr = _run_native(self.ctx, optimizer_kind, solver_kind, Jd, self.x, self.fcur,
                                  self._fg[0], self._fg[1], self.model, x_tol, f_tol, g_tol,
                                  iterations, delta, lower, upper, trace, self.n, allreduce=allreduce,
                                  row_allreduce=row_allreduce, row_allreduce_user=row_allreduce_user, global_rows=global_rows)
        check(st)
        r = LeastSquaresResult()
        r.optimizer = "LevenbergMarquardt" if res.optimizer == _lib.LEVENBERG_MARQUARDT else "Dogleg"
        r.ssr, r.iterations = float(res.ssr), res.iterations
        r.converged = bool(res.converged)
        r.x_converged, r.f_converged, r.g_converged = bool(res.x_converged), bool(res.f_converged), bool(res.g_converged)
        r.x_tol, r.f_tol, r.g_tol = x_tol, f_tol, g_tol
        r.f_calls, r.g_calls, r.mul_calls = res.f_calls, res.g_calls, res.mul_calls
        r.seconds, r.lsmr_iterations = res.seconds, int(res.lsmr_iterations)
        r.trace = tr
        r.minimizer = self.x.get() if fetch_x else None
        return r

    def optimize_batched(self, optimizer_kind=_lib.LEVENBERG_MARQUARDT, solver_kind=_lib.CHOLESKY, x_tol=1e-8, f_tol=1e-8,
                         g_tol=1e-8, iterations=1000, delta=None, lower=None, upper=None, trace=False, fetch_x=True):
        """The twin of optimize() on a blockdiag= problem: one trust region per block (lsq_optimize_batched), f! / g! on the
        device, no host callbacks.  Returns an api.BatchedResult."""
        if self.blockdiag is None:
            raise _lib.ArgumentError(_lib.EARG, "optimize_batched needs a problem built with blockdiag=(nblocks, mb, nb)")
        if self._fg is None:
            L = lib()
            self._Jd = _Handle(self.J)
            self._fg = (L.lsq_model_f(), L.lsq_model_g())
        name = "LevenbergMarquardt" if optimizer_kind == _lib.LEVENBERG_MARQUARDT else "Dogleg"
        st, r = _run_native_batched(self.ctx, optimizer_kind, solver_kind, self.J, self.blockdiag, self.x, self.fcur,
                                    self._fg[0], self._fg[1], self.model, x_tol, f_tol, g_tol, iterations, delta, lower, upper,
                                    trace, name)
        check(st)
        r.minimizer = self.x.get() if fetch_x else None
        return r

    def paths(self):
        """What the solves on this problem ran on (lsq_model_paths): sliced layouts built, LSMR driver of the latest solve,
        launches of LM's one-pass tail so far."""
        rows, cols, lpath, pairs = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        check(lib().lsq_model_paths(self.model, C.byref(rows), C.byref(cols), C.byref(lpath), C.byref(pairs)))
        return dict(sliced_rows=bool(rows.value), sliced_cols=bool(cols.value), pair_tails=pairs.value,
                    lsmr_path={0: None, 1: "reference-order", 2: "four-launch", 3: "three-launch", 4: "general"}[lpath.value])

    def close(self):
        L = lib()
        if self.model:
            L.lsq_model_destroy(self.model)
            self.model = None
        if self.J:
            L.lsq_mat_destroy(self.J)
            self.J = None
